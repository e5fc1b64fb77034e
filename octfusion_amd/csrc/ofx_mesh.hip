// Marching cubes over batched SDF lattices (mesh export of the generate path: the reference's export_mesh,
// models/octfusion_model_union.py:435-468, skimage marching_cubes + trimesh on the host).
//
// Contract (include/ofx.h; restated by tests/mc_oracle.py): lattice sdf [B, R, R, R] fp32, x slowest.  A corner is
// inside iff v < level.  One vertex per lattice edge with exactly one inside endpoint, owned by the lower endpoint and
// numbered by (owner linear index, axis x/y/z); triangles from the table of tools/gen_mc_table.py, numbered by (cell
// linear index, table order).  Order comes from scans, never from atomics: the output is bitwise reproducible.
// Limits: 2 <= size <= 512, 1 <= batch <= 65535 (the second grid dimension of the count pass) and
// batch * size^3 * 5 <= INT32_MAX; ofx_mc_ws_bytes returns 0 and the entries OFX_EINVAL outside.  The crossing
// parameter t = (level - v0) / (v1 - v0) is plain fp32: when v1 - v0 overflows to +-inf, t is +-0 and the vertex is the
// owner point.
//
// Passes.  The lattice is cut into chunks of MC_CHUNK consecutive points (one block each).
//   count  (ofx_mc_count): every block counts its vertices, triangles and non-finite cells -> three int32 per block;
//          ofx_scan_i32 over the block totals of the whole batch; a finishing kernel writes the per-shape counts.
//   emit   (ofx_mc_emit), per shape, so the shape's lattice is re-read from the Infinity Cache:
//          vertices: a block with vertices recomputes its edge crossings, ranks them with ballots (LDS across waves),
//                    writes the positions and, for every point that owns a vertex, its first vertex id and crossing
//                    mask into the id map (one uint32 per point, written only there);
//          triangles: a block with triangles recomputes the cube indices and looks the seven owner points of its
//                    cells' edges up in the id map.
//   Blocks without output return after reading two scanned totals: the emit pass reads the lattice only near the
//   surface.
#include "ofx_common.h"
#include "ofx_mc_table.h"

#include <cmath>

namespace {

constexpr int MC_T = 256;                 // threads per block (4 waves)
constexpr int MC_ITER = 4;                // points per thread
constexpr int MC_CHUNK = MC_T * MC_ITER;  // points per block
constexpr int MC_MAX_SIZE = 512;          // id map: 29-bit vertex id + 3-bit crossing mask; 3 * 512^3 < 2^29
constexpr int MC_MAX_BATCH = 65535;       // the count pass puts the shape into the grid's y dimension
constexpr uint32_t MC_ID_MASK = (1u << 29) - 1;

struct McWs {
  int32_t* cnt;   // [3][n]   vertices, triangles, non-finite cells per block
  int32_t* pre;   // [3][n+1] exclusive scans of cnt
  void* scan_ws;  // ofx_scan_i32 workspace for n
  uint32_t* ids;  // [R^3]    id map of the shape being emitted
};

inline size_t mc_align(size_t b) { return (b + 255) & ~(size_t)255; }

inline int64_t mc_nblk(int size) { return ofx_cdiv((int64_t)size * size * size, MC_CHUNK); }

size_t mc_layout(int batch, int size, char* base, McWs* w) {
  const int64_t n = (int64_t)batch * mc_nblk(size);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += mc_align(bytes);
    return p;
  };
  McWs l;
  l.cnt = (int32_t*)take(3 * n * sizeof(int32_t));
  l.pre = (int32_t*)take(3 * (n + 1) * sizeof(int32_t));
  l.scan_ws = take(ofx_scan_ws_bytes(n));
  l.ids = (uint32_t*)take((size_t)size * size * size * sizeof(uint32_t));
  if (w) *w = l;
  return off;
}

bool mc_valid(int batch, int size) {
  // every count of the batch goes through one int32 scan: bound the worst case (5 triangles per cell); the batch is
  // a grid dimension of the count pass (and the emit pass launches per shape), so small lattices are bounded by it
  return batch >= 1 && batch <= MC_MAX_BATCH && size >= 2 && size <= MC_MAX_SIZE &&
         (int64_t)batch * size * size * size * OFX_MC_MAX_TRI <= INT32_MAX;
}

// Crossing mask (bit a: the +axis-a edge of point p crosses) and cube index of the cell whose lower corner is p
// (0 where there is no such cell); bad = the cell has a non-finite corner.
__device__ __forceinline__ void mc_eval(const float* __restrict__ s, int R, int p, float level, int& mask, int& ci,
                                        int& bad) {
  const int RR = R * R;
  const int x = p / RR, y = (p / R) % R, z = p % R;
  const bool hx = x < R - 1, hy = y < R - 1, hz = z < R - 1;
  const float v000 = s[p];
  const float v001 = hz ? s[p + 1] : 0.f, v010 = hy ? s[p + R] : 0.f, v100 = hx ? s[p + RR] : 0.f;
  const int i000 = v000 < level, i001 = v001 < level, i010 = v010 < level, i100 = v100 < level;
  mask = (hx && i100 != i000 ? 1 : 0) | (hy && i010 != i000 ? 2 : 0) | (hz && i001 != i000 ? 4 : 0);
  ci = 0;
  bad = 0;
  if (hx && hy && hz) {
    const float v011 = s[p + R + 1], v101 = s[p + RR + 1], v110 = s[p + RR + R], v111 = s[p + RR + R + 1];
    ci = i000 | (i001 << 1) | (i010 << 2) | ((v011 < level) << 3) | (i100 << 4) | ((v101 < level) << 5) |
         ((v110 < level) << 6) | ((v111 < level) << 7);
    bad = !(isfinite(v000) && isfinite(v001) && isfinite(v010) && isfinite(v011) && isfinite(v100) &&
            isfinite(v101) && isfinite(v110) && isfinite(v111));
  }
}

// Exclusive block-wide rank of `val` (< 2^BITS) in thread order, and the block total; ballots per bit within a wave,
// wave totals through LDS.  All threads of the block must call it.
template <int BITS>
__device__ __forceinline__ int mc_block_rank(int val, int* lds4, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t lt = (1ull << lane) - 1ull;
  int rank = 0, wsum = 0;
#pragma unroll
  for (int b = 0; b < BITS; ++b) {
    const uint64_t m = __ballot((val >> b) & 1);
    rank += __popcll(m & lt) << b;
    wsum += __popcll(m) << b;
  }
  if (lane == 0) lds4[wave] = wsum;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < MC_T / 64; ++w) {
    const int t = lds4[w];
    before += w < wave ? t : 0;
    total += t;
  }
  __syncthreads();
  return before + rank;
}

__global__ __launch_bounds__(MC_T) void mc_count_kernel(const float* __restrict__ sdf, int R, int n3, int nblk,
                                                        float level, int32_t* __restrict__ cnt, int64_t n) {
  __shared__ uint8_t ntri[256];
  __shared__ int red[3][MC_T / 64];
  ntri[threadIdx.x] = OFX_MC_NTRI[threadIdx.x];
  __syncthreads();
  const int b = blockIdx.y, blk = blockIdx.x;
  const float* s = sdf + (int64_t)b * n3;
  int nv = 0, nt = 0, nb = 0;
#pragma unroll
  for (int it = 0; it < MC_ITER; ++it) {
    const int p = blk * MC_CHUNK + it * MC_T + threadIdx.x;
    if (p < n3) {
      int mask, ci, bad;
      mc_eval(s, R, p, level, mask, ci, bad);
      nv += __popc(mask);
      nt += ntri[ci];
      nb += bad;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nv += __shfl_xor(nv, o);
    nt += __shfl_xor(nt, o);
    nb += __shfl_xor(nb, o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[0][wave] = nv;
    red[1][wave] = nt;
    red[2][wave] = nb;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < MC_T / 64; ++w) t += red[threadIdx.x][w];
    cnt[threadIdx.x * n + (int64_t)b * nblk + blk] = t;
  }
}

__global__ void mc_counts_kernel(const int32_t* __restrict__ pre, int64_t n, int batch, int nblk,
                                 int64_t* __restrict__ counts) {
  for (int i = threadIdx.x; i < batch * 3; i += blockDim.x) {
    const int b = i / 3, k = i % 3;
    const int32_t* q = pre + k * (n + 1);
    counts[i] = (int64_t)q[(int64_t)(b + 1) * nblk] - q[(int64_t)b * nblk];
  }
}

__global__ __launch_bounds__(MC_T) void mc_vert_kernel(const float* __restrict__ s, int R, int n3, int nblk, int b,
                                                       float level, float step, float bbmin, float scale,
                                                       const int32_t* __restrict__ pre_v,
                                                       const int64_t* __restrict__ vert_off,
                                                       float* __restrict__ verts, uint32_t* __restrict__ ids) {
  __shared__ int lds4[MC_T / 64];
  const int64_t g = (int64_t)b * nblk + blockIdx.x;
  if (pre_v[g + 1] == pre_v[g]) return;                 // no vertex in this chunk (uniform over the block)
  int run = pre_v[g] - pre_v[(int64_t)b * nblk];        // shape-relative id of the chunk's first vertex
  float* out = verts + vert_off[b] * 3;
  const int RR = R * R;
#pragma unroll 1
  for (int it = 0; it < MC_ITER; ++it) {
    const int p = blockIdx.x * MC_CHUNK + it * MC_T + threadIdx.x;
    int mask = 0;
    if (p < n3) {
      int ci, bad;
      mc_eval(s, R, p, level, mask, ci, bad);
    }
    int total;
    const int id = run + mc_block_rank<2>(__popc(mask), lds4, total);
    if (mask) {
      ids[p] = (uint32_t)id | ((uint32_t)mask << 29);
      const int x = p / RR, y = (p / R) % R, z = p % R;
      const float v0 = s[p];
      int k = id;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        if (!((mask >> a) & 1)) continue;
        const float v1 = s[p + (a == 0 ? RR : a == 1 ? R : 1)];
        const float t = (level - v0) / (v1 - v0);
        float px = (float)x, py = (float)y, pz = (float)z;
        if (a == 0) px = px + t;
        else if (a == 1) py = py + t;
        else pz = pz + t;
        float* o = out + (int64_t)k * 3;
        o[0] = __fmul_rn(__fadd_rn(__fmul_rn(px, step), bbmin), scale);
        o[1] = __fmul_rn(__fadd_rn(__fmul_rn(py, step), bbmin), scale);
        o[2] = __fmul_rn(__fadd_rn(__fmul_rn(pz, step), bbmin), scale);
        ++k;
      }
    }
    run += total;
  }
}

__global__ __launch_bounds__(MC_T) void mc_tri_kernel(const float* __restrict__ s, int R, int n3, int nblk, int b,
                                                      float level, const int32_t* __restrict__ pre_t,
                                                      const int64_t* __restrict__ tri_off,
                                                      const uint32_t* __restrict__ ids, int32_t* __restrict__ faces) {
  __shared__ int lds4[MC_T / 64];
  __shared__ int8_t tab[256 * OFX_MC_TRI_STRIDE];
  __shared__ uint8_t ntri[256];
  const int64_t g = (int64_t)b * nblk + blockIdx.x;
  if (pre_t[g + 1] == pre_t[g]) return;
  for (int i = threadIdx.x; i < 256 * OFX_MC_TRI_STRIDE; i += MC_T) tab[i] = (&OFX_MC_TRI[0][0])[i];
  ntri[threadIdx.x] = OFX_MC_NTRI[threadIdx.x];
  __syncthreads();
  int run = pre_t[g] - pre_t[(int64_t)b * nblk];
  int32_t* out = faces + tri_off[b] * 3;
  const int RR = R * R;
#pragma unroll 1
  for (int it = 0; it < MC_ITER; ++it) {
    const int p = blockIdx.x * MC_CHUNK + it * MC_T + threadIdx.x;
    int ci = 0;
    if (p < n3) {
      int mask, bad;
      mc_eval(s, R, p, level, mask, ci, bad);
    }
    const int nt = ntri[ci];
    int total;
    const int first = run + mc_block_rank<3>(nt, lds4, total);
    const int8_t* row = tab + ci * OFX_MC_TRI_STRIDE;
    for (int j = 0; j < 3 * nt; ++j) {
      const int e = row[j];
      const int axis = e >> 2, hi = (e >> 1) & 1, lo = e & 1;
      const int dx = axis == 0 ? 0 : hi, dy = axis == 0 ? hi : axis == 1 ? 0 : lo, dz = axis == 2 ? 0 : lo;
      const uint32_t w = ids[p + dx * RR + dy * R + dz];
      const int id = (int)(w & MC_ID_MASK) + __popc((w >> 29) & ((1u << axis) - 1u));
      out[(int64_t)first * 3 + j] = id;
    }
    run += total;
  }
}

}  // namespace

extern "C" size_t ofx_mc_ws_bytes(int batch, int size) {
  if (!mc_valid(batch, size)) return 0;
  return mc_layout(batch, size, nullptr, nullptr);
}

extern "C" int ofx_mc_count(const float* sdf, int batch, int size, float level, void* ws, int64_t* counts,
                            void* stream) {
  if (!mc_valid(batch, size) || !sdf || !ws || !counts || !std::isfinite(level)) return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  McWs w;
  mc_layout(batch, size, (char*)ws, &w);
  const int nblk = (int)mc_nblk(size), n3 = size * size * size;
  const int64_t n = (int64_t)batch * nblk;
  mc_count_kernel<<<dim3(nblk, batch), MC_T, 0, st>>>(sdf, size, n3, nblk, level, w.cnt, n);
  OFX_LAUNCH_CHECK();
  for (int k = 0; k < 3; ++k) {
    const int rc = ofx_scan_i32(w.cnt + k * n, w.pre + k * (n + 1), n, w.scan_ws, stream);
    if (rc) return rc;
  }
  mc_counts_kernel<<<1, 256, 0, st>>>(w.pre, n, batch, nblk, counts);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" int ofx_mc_emit(const float* sdf, int batch, int size, float level, float step, float bbmin, float scale,
                           void* ws, const int64_t* vert_off, const int64_t* tri_off, float* verts, int32_t* faces,
                           void* stream) {
  if (!mc_valid(batch, size) || !sdf || !ws || !vert_off || !tri_off || !verts || !faces || !std::isfinite(level))
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  McWs w;
  mc_layout(batch, size, (char*)ws, &w);
  const int nblk = (int)mc_nblk(size), n3 = size * size * size;
  const int64_t n = (int64_t)batch * nblk;
  for (int b = 0; b < batch; ++b) {          // shape-major: the triangle pass re-reads what the vertex pass cached
    const float* s = sdf + (int64_t)b * n3;
    mc_vert_kernel<<<nblk, MC_T, 0, st>>>(s, size, n3, nblk, b, level, step, bbmin, scale, w.pre, vert_off, verts,
                                          w.ids);
    mc_tri_kernel<<<nblk, MC_T, 0, st>>>(s, size, n3, nblk, b, level, w.pre + (n + 1), tri_off, w.ids, faces);
  }
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" int ofx_mc_table_host(int8_t* tri_table, uint8_t* ntri) {
  if (!tri_table || !ntri) return OFX_EINVAL;
  for (int c = 0; c < 256; ++c) {
    ntri[c] = OFX_MC_NTRI[c];
    for (int j = 0; j < 16; ++j) tri_table[c * 16 + j] = j < OFX_MC_TRI_STRIDE ? OFX_MC_TRI[c][j] : -1;
  }
  return OFX_OK;
}

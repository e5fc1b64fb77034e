// Mesh simplification by vertex clustering with quadric-error placement (Lindstrom 2000, "Out-of-core simplification
// of large polygonal models"): the decimation the reference's users run on the host (trimesh / meshlab) after
// export_mesh, one mesh at a time.  A uniform grid over the mesh's bounding box; every occupied cell becomes one
// vertex, placed where the summed squared distances to the planes of the cell's faces are least; faces that keep three
// different cells survive.  No priority queue and no collapse order: two stable sorts per side, scans, one 3 x 3 solve
// per cell, and the output is a pure function of the mesh.
//
// Contract (include/ofx.h; restated by tests/simplify_oracle.py).  The mesh is in the layout
// ofx_mc_emit writes: verts [V, 3] fp32, faces [F, 3] int32 local to each shape, vert_off / tri_off int64
// [batch + 1].  All arithmetic below is fp64 (contraction off: the cell index is IEEE subtract / divide / floor and
// must agree with numpy exactly).
//   grid      lo / hi = exact min / max of ALL vertices of the shape, side = max axis of hi - lo, h = side / cells or
//             h = cell_size; cell = floor((v - lo) / h), clamped to cells - 1 (cells) or flagged >= 1024 (cell_size);
//             side == 0: cell (0, 0, 0).  A shape with a NaN or infinite coordinate in ANY of its vertices (used by a
//             face or not) is refused in both modes: bit 1 of status[1], counts column 7; it is left as one cluster
//             in cell (0, 0, 0) and its outputs are not to be used; the other shapes of the batch are not affected
//   clusters  occupied cells in ascending (ix, iy, iz); m = mean of the cluster's vertices, c = lo + (cell + 0.5) h
//   quadrics  face t, once per distinct cluster k of its corners: q_i = p_i - c_k, n = (q1 - q0) x (q2 - q0),
//             A_k += n n^T, b_k += (n . q0) n
//   placement lam = reg trace(A) / 3; trace == 0: x = m; else (A + lam I) y = b + lam (m - c) by Cholesky,
//             x = clamp(y + c, the cell's box); one rounding to fp32
//   faces     corners -> clusters; kept iff the three differ; rotated lowest first; the first of equal rotated triples
//             (in input order) survives; input order kept
//   compact   clusters no surviving face uses are dropped
//
// Passes (g = vert_off[b] + v; every pass after `check` returns at once when a face index is out of range):
//   keys      check F; box V (order-preserving uint32 min / max atomics, one set per 1024-vertex chunk in one shape);
//             grid B (a box entry that is not finite <=> a non-finite vertex: the encoding sorts NaN outside the
//             infinities); key[g] = b << 30 | ix << 20 | iy << 10 | iz
//   vsort     stable radix sort of (key, g) over the live bits; head flags + scan -> cluster id of every vertex (global,
//             ascending in (shape, cell)), cluster start in the sorted order, clusters before every shape
//   isort     per face three (cluster, face) slots, repeats replaced by a sentinel that sorts last; stable radix sort by
//             cluster -> every cluster owns a contiguous segment in ascending face id; the ends of the runs give
//             every cluster its segment bounds
//   solve     one wave per cluster: lanes stride the vertex segment (mean) and the incidence segment (quadric) from the
//             segment's own start, a fixed xor butterfly combines them, lane 0 solves and writes
//   faces     distinct flags + scan (collapsed counts); two stable sorts of the rotated triples (third entry, then
//             first << 32 | second) with the face id as value; "first of its run" scattered back; scan in input order;
//             used-cluster flags + scan; per-shape counts
//   extract   (after the caller's readback) vertices and faces compacted through the scans
// Determinism: no floating-point atomics.  A lane's share of a segment depends on the position inside the segment only,
// the segment's order on the shape's own vertex and face ids (stable sorts), so a mesh gives the same bytes alone or
// anywhere in a batch.
#include <hipcub/hipcub.hpp>

#include "ofx_common.h"

#include <climits>

#pragma clang fp contract(off)

namespace {

constexpr int SP_T = 256;
constexpr int SP_MAX_CELLS = 1024;
constexpr int SP_COUNTS = 8;     // clusters, kept vertices, kept faces, collapsed, duplicate, bad index, overflow,
                                 // non-finite vertex
constexpr int SP_GRID = 5;       // lo[3], h, side
constexpr int SP_STAGES = 5;

struct SpWs {
  uint32_t* box;             // [batch, 6]   encoded min[3], max[3]
  double* grid;              // [batch, 5]
  int32_t* coff;             // [batch + 1]  clusters before every shape
  uint64_t *key_a, *key_b;   // [V]          vertex keys, unsorted / sorted
  int32_t *idx_a, *idx_b;    // [V]          vertex ids
  int32_t* flag;             // [V]          head flags, later used-cluster flags
  int32_t* pre;              // [V + 1]      scan of the head flags (pre[V] = clusters)
  int32_t* upre;             // [V + 1]      scan of the used flags
  int32_t* cstart;           // [V + 1]      first sorted position of every cluster
  int32_t* cov;              // [V]          cluster of every vertex
  int32_t *istart, *iend;    // [V]          every cluster's segment of the sorted incidences
  float* pos;                // [V, 3]       cluster positions
  uint32_t *ik_a, *ik_b;     // [3F]         incidence keys; later the faces' third entries
  int32_t *iv_a, *iv_b;      // [3F]         incidence faces; later face ids
  uint64_t *fk_a, *fk_b;     // [F]          first << 32 | second of the rotated triples
  int32_t* fflag;            // [F]          distinct flags, later keep flags
  int32_t* fpre;             // [F + 1]
  void* scan_ws;
  void* sort_ws;
  size_t sort_bytes;
};

inline size_t sp_align(size_t b) { return (b + 255) & ~(size_t)255; }

bool sp_valid(int64_t V, int64_t F, int batch) {
  return batch >= 1 && V >= 1 && F >= 1 && V < INT32_MAX && F <= INT32_MAX / 3;
}

inline int sp_bits(uint64_t x) {       // bits needed to hold x
  int n = 0;
  while (x) {
    ++n;
    x >>= 1;
  }
  return n;
}

template <typename KeyT>
size_t sp_sort_query(int64_t n) {
  size_t bytes = 0;
  const KeyT* kin = nullptr;
  KeyT* kout = nullptr;
  const int32_t* vin = nullptr;
  int32_t* vout = nullptr;
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, kin, kout, vin, vout, (int)n, 0, (int)sizeof(KeyT) * 8,
                                         (hipStream_t)0) != hipSuccess)
    return 0;
  return bytes;
}

// one temporary buffer for the three sorts: vertex keys, incidences, face pairs
size_t sp_sort_bytes(int64_t V, int64_t F) {
  const size_t a = sp_sort_query<uint64_t>(V), b = sp_sort_query<uint32_t>(3 * F), c = sp_sort_query<uint64_t>(F);
  const size_t ab = a > b ? a : b;
  return (ab > c ? ab : c) + 16;
}

size_t sp_layout(int64_t V, int64_t F, int batch, char* base, SpWs* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += sp_align(bytes);
    return p;
  };
  SpWs l;
  l.box = (uint32_t*)take((size_t)batch * 6 * 4);
  l.grid = (double*)take((size_t)batch * SP_GRID * 8);
  l.coff = (int32_t*)take((size_t)(batch + 1) * 4);
  l.key_a = (uint64_t*)take((size_t)V * 8);
  l.key_b = (uint64_t*)take((size_t)V * 8);
  l.idx_a = (int32_t*)take((size_t)V * 4);
  l.idx_b = (int32_t*)take((size_t)V * 4);
  l.flag = (int32_t*)take((size_t)V * 4);
  l.pre = (int32_t*)take((size_t)(V + 1) * 4);
  l.upre = (int32_t*)take((size_t)(V + 1) * 4);
  l.cstart = (int32_t*)take((size_t)(V + 1) * 4);
  l.cov = (int32_t*)take((size_t)V * 4);
  l.istart = (int32_t*)take((size_t)V * 4);      // adjacent: one memset clears both
  l.iend = (int32_t*)take((size_t)V * 4);
  l.pos = (float*)take((size_t)V * 3 * 4);
  l.ik_a = (uint32_t*)take((size_t)F * 3 * 4);
  l.ik_b = (uint32_t*)take((size_t)F * 3 * 4);
  l.iv_a = (int32_t*)take((size_t)F * 3 * 4);
  l.iv_b = (int32_t*)take((size_t)F * 3 * 4);
  l.fk_a = (uint64_t*)take((size_t)F * 8);
  l.fk_b = (uint64_t*)take((size_t)F * 8);
  l.fflag = (int32_t*)take((size_t)F * 4);
  l.fpre = (int32_t*)take((size_t)(F + 1) * 4);
  l.scan_ws = take(ofx_scan_ws_bytes(V > F ? V : F));
  l.sort_bytes = sp_sort_bytes(V, F);
  l.sort_ws = take(l.sort_bytes);
  if (w) *w = l;
  return off;
}

// the shape that owns item i: the largest b with off[b] <= i (empty shapes have equal offsets and own nothing)
__device__ __forceinline__ int sp_shape(const int64_t* __restrict__ off, int batch, int64_t i) {
  int lo = 0, hi = batch;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// order-preserving uint32 image of an fp32 value (-0 below +0)
__device__ __forceinline__ uint32_t sp_enc(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sp_dec(uint32_t e) {
  return __uint_as_float((e & 0x80000000u) ? (e ^ 0x80000000u) : ~e);
}

#define SP_LOOP(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

// ---- keys ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_T) void sp_check_kernel(const int32_t* __restrict__ faces,
                                                        const int64_t* __restrict__ vert_off,
                                                        const int64_t* __restrict__ tri_off, int batch, int64_t V,
                                                        int64_t F, int64_t* __restrict__ counts, int32_t* status) {
  // the offsets themselves: ascending, from 0 to the totals the host sized everything by
  bool ok = vert_off[0] == 0 && tri_off[0] == 0 && vert_off[batch] == V && tri_off[batch] == F;
  for (int b = 0; b < batch && ok; ++b) ok = vert_off[b] <= vert_off[b + 1] && tri_off[b] <= tri_off[b + 1];
  if (!ok) {                       // every thread sees the same tables: nobody follows them
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 2);
    return;
  }
  SP_LOOP(f, F) {
    const int b = sp_shape(tri_off, batch, f);
    const int64_t nv = vert_off[b + 1] - vert_off[b];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int64_t i = faces[f * 3 + j];
      bad = bad || i < 0 || i >= nv;
    }
    if (bad) {
      atomicOr(status, 1);
      counts[(int64_t)b * SP_COUNTS + 5] = 1;      // every writer stores the same value
    }
  }
}

__global__ void sp_box_init_kernel(uint32_t* __restrict__ box, int batch) {
  SP_LOOP(i, (int64_t)batch * 6) box[i] = (i % 6) < 3 ? 0xFFFFFFFFu : 0u;
}

// Every wave owns chunks of SP_BOX_CHUNK consecutive vertices; a lane keeps a running box over its share of the chunk and
// flushes it only when the shape changes.  A chunk that lies in one shape -- nearly every chunk -- is then reduced
// across the wave and costs one set of atomics.
constexpr int SP_BOX_CHUNK = 64 * 16;

__device__ __forceinline__ void sp_box_flush(uint32_t* __restrict__ box, int b, const uint32_t* mn, const uint32_t* mx) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    atomicMin(box + (int64_t)b * 6 + a, mn[a]);
    atomicMax(box + (int64_t)b * 6 + 3 + a, mx[a]);
  }
}

__global__ __launch_bounds__(SP_T) void sp_box_kernel(const float* __restrict__ verts,
                                                      const int64_t* __restrict__ vert_off, int batch, int64_t V,
                                                      uint32_t* __restrict__ box, const int32_t* __restrict__ status) {
  if (status[0]) return;
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (SP_T / 64);
  for (int64_t c0 = ((int64_t)blockIdx.x * (SP_T / 64) + (threadIdx.x >> 6)) * SP_BOX_CHUNK; c0 < V;
       c0 += waves * SP_BOX_CHUNK) {
    int cur = -1;
    uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u};
    for (int it = 0; it < SP_BOX_CHUNK / 64; ++it) {
      const int64_t g = c0 + it * 64 + lane;
      if (g >= V) continue;
      const int b = sp_shape(vert_off, batch, g);
      if (b != cur) {
        if (cur >= 0) sp_box_flush(box, cur, mn, mx);
        cur = b;
#pragma unroll
        for (int a = 0; a < 3; ++a) mn[a] = 0xFFFFFFFFu, mx[a] = 0u;
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const uint32_t e = sp_enc(verts[g * 3 + a]);
        mn[a] = e < mn[a] ? e : mn[a];
        mx[a] = e > mx[a] ? e : mx[a];
      }
    }
    int bmax = cur;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int t = __shfl_xor(bmax, o);
      bmax = t > bmax ? t : bmax;
    }
    if (__all(cur < 0 || cur == bmax)) {       // idle lanes hold the neutral box
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const uint32_t tn = __shfl_xor(mn[a], o), tx = __shfl_xor(mx[a], o);
          mn[a] = tn < mn[a] ? tn : mn[a];
          mx[a] = tx > mx[a] ? tx : mx[a];
        }
      }
      if (lane == 0 && bmax >= 0) sp_box_flush(box, bmax, mn, mx);
    } else if (cur >= 0) {
      sp_box_flush(box, cur, mn, mx);
    }
  }
}

__global__ void sp_grid_kernel(const uint32_t* __restrict__ box, const int64_t* __restrict__ vert_off, int batch,
                               int cells, double cell_size, double* __restrict__ grid,
                               int64_t* __restrict__ counts, int32_t* status) {
  if (status[0]) return;
  SP_LOOP(b, batch) {
    double* gr = grid + b * SP_GRID;
    if (vert_off[b + 1] == vert_off[b]) {
      for (int a = 0; a < SP_GRID; ++a) gr[a] = 0.0;
      continue;
    }
    // Every vertex of the shape went into the box, and the encoding puts -NaN below -inf and +NaN above +inf: the
    // shape has a non-finite coordinate iff one of its six box entries is not finite.
    bool finite = true;
#pragma unroll
    for (int a = 0; a < 6; ++a) finite = finite && isfinite(sp_dec(box[b * 6 + a]));
    if (!finite) {                     // refused: flagged, and left as one cluster in cell (0, 0, 0) (side == 0)
      atomicOr(status + 1, 2);
      counts[b * SP_COUNTS + 7] = 1;
      for (int a = 0; a < SP_GRID; ++a) gr[a] = 0.0;
      continue;
    }
    double side = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double lo = (double)sp_dec(box[b * 6 + a]), hi = (double)sp_dec(box[b * 6 + 3 + a]);
      gr[a] = lo;
      const double d = hi - lo;
      side = a == 0 || d > side ? d : side;
    }
    gr[3] = cells > 0 ? side / (double)cells : cell_size;
    gr[4] = side;
  }
}

__global__ __launch_bounds__(SP_T) void sp_keys_kernel(const float* __restrict__ verts,
                                                       const int64_t* __restrict__ vert_off, int batch, int64_t V,
                                                       int cells, const double* __restrict__ grid,
                                                       uint64_t* __restrict__ key, int32_t* __restrict__ idx,
                                                       int64_t* __restrict__ counts, int32_t* status) {
  if (status[0]) return;
  SP_LOOP(g, V) {
    const int b = sp_shape(vert_off, batch, g);
    const double* gr = grid + (int64_t)b * SP_GRID;
    const double h = gr[3], side = gr[4];
    uint32_t c[3];
    bool over = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double d = side == 0.0 ? 0.0 : floor(((double)verts[g * 3 + a] - gr[a]) / h);
      int i;
      if (cells > 0) {
        i = d >= (double)(cells - 1) ? cells - 1 : (d >= 0.0 ? (int)d : 0);
      } else if (!(d < (double)SP_MAX_CELLS)) {          // too many cells (or not a number)
        over = true;
        i = SP_MAX_CELLS - 1;
      } else {
        i = d >= 0.0 ? (int)d : 0;
      }
      c[a] = (uint32_t)i;
    }
    if (over) {
      atomicOr(status + 1, 1);
      counts[(int64_t)b * SP_COUNTS + 6] = 1;          // every writer stores the same value
    }
    key[g] = ((uint64_t)b << 30) | ((uint64_t)c[0] << 20) | ((uint64_t)c[1] << 10) | c[2];
    idx[g] = (int32_t)g;
  }
}

// ---- vsort -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_T) void sp_heads_kernel(const uint64_t* __restrict__ key, int64_t V,
                                                        int32_t* __restrict__ flag,
                                                        const int32_t* __restrict__ status) {
  if (status[0]) return;
  SP_LOOP(i, V) flag[i] = i == 0 || key[i] != key[i - 1];
}

__global__ __launch_bounds__(SP_T) void sp_ids_kernel(const int32_t* __restrict__ idx,
                                                      const int32_t* __restrict__ flag,
                                                      const int32_t* __restrict__ pre,
                                                      const int64_t* __restrict__ vert_off, int batch, int64_t V,
                                                      int32_t* __restrict__ cov, int32_t* __restrict__ cstart,
                                                      int32_t* __restrict__ coff,
                                                      const int32_t* __restrict__ status) {
  if (status[0]) return;
  // the sort puts shape b's vertices at the sorted positions [vert_off[b], vert_off[b + 1])
  if (blockIdx.x == 0)
    for (int b = threadIdx.x; b <= batch; b += blockDim.x) coff[b] = pre[vert_off[b]];
  SP_LOOP(i, V) {
    const int k = pre[i + 1] - 1;
    cov[idx[i]] = k;
    if (flag[i]) cstart[k] = (int32_t)i;
    if (i == V - 1) cstart[k + 1] = (int32_t)V;
  }
}

// ---- isort -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_T) void sp_incidence_kernel(const int32_t* __restrict__ faces,
                                                            const int32_t* __restrict__ cov,
                                                            const int64_t* __restrict__ vert_off,
                                                            const int64_t* __restrict__ tri_off, int batch, int64_t F,
                                                            uint32_t sentinel, uint32_t* __restrict__ ik,
                                                            int32_t* __restrict__ iv,
                                                            const int32_t* __restrict__ status) {
  if (status[0]) return;
  SP_LOOP(f, F) {
    const int64_t vo = vert_off[sp_shape(tri_off, batch, f)];
    const uint32_t k0 = (uint32_t)cov[vo + faces[f * 3]], k1 = (uint32_t)cov[vo + faces[f * 3 + 1]],
                   k2 = (uint32_t)cov[vo + faces[f * 3 + 2]];
    ik[f * 3] = k0;
    ik[f * 3 + 1] = k1 != k0 ? k1 : sentinel;
    ik[f * 3 + 2] = (k2 != k0 && k2 != k1) ? k2 : sentinel;
#pragma unroll
    for (int j = 0; j < 3; ++j) iv[f * 3 + j] = (int32_t)f;
  }
}

// first and one-past-last sorted incidence of every cluster (both zero, from the memset, for a cluster no face touches)
__global__ __launch_bounds__(SP_T) void sp_segments_kernel(const uint32_t* __restrict__ ik, int64_t n,
                                                           uint32_t sentinel, int32_t* __restrict__ istart,
                                                           int32_t* __restrict__ iend,
                                                           const int32_t* __restrict__ status) {
  if (status[0]) return;
  SP_LOOP(i, n) {
    const uint32_t k = ik[i];
    if (k >= sentinel) continue;
    if (i == 0 || ik[i - 1] != k) istart[k] = (int32_t)i;
    if (i == n - 1 || ik[i + 1] != k) iend[k] = (int32_t)(i + 1);
  }
}

// ---- solve -----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double sp_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// (A + lam I) y = r for a symmetric positive definite A = {xx, xy, xz, yy, yz, zz}, by Cholesky
__device__ __forceinline__ void sp_solve3(const double* A, const double* r, double* y) {
  const double l00 = sqrt(A[0]);
  const double l10 = A[1] / l00, l20 = A[2] / l00;
  const double l11 = sqrt(A[3] - l10 * l10);
  const double l21 = (A[4] - l20 * l10) / l11;
  const double l22 = sqrt(A[5] - l20 * l20 - l21 * l21);
  const double z0 = r[0] / l00;
  const double z1 = (r[1] - l10 * z0) / l11;
  const double z2 = (r[2] - l20 * z0 - l21 * z1) / l22;
  y[2] = z2 / l22;
  y[1] = (z1 - l21 * y[2]) / l11;
  y[0] = (z0 - l10 * y[1] - l20 * y[2]) / l00;
}

__global__ __launch_bounds__(SP_T) void sp_solve_kernel(const float* __restrict__ verts,
                                                        const int32_t* __restrict__ faces,
                                                        const int64_t* __restrict__ vert_off, int64_t V, int64_t F,
                                                        double reg, const double* __restrict__ grid,
                                                        const uint64_t* __restrict__ key,
                                                        const int32_t* __restrict__ idx,
                                                        const int32_t* __restrict__ pre,
                                                        const int32_t* __restrict__ cstart,
                                                        const int32_t* __restrict__ istart,
                                                        const int32_t* __restrict__ iend,
                                                        const int32_t* __restrict__ iv, float* __restrict__ pos,
                                                        const int32_t* __restrict__ status) {
  if (status[0]) return;
  const int lane = threadIdx.x & 63;
  const int64_t K = pre[V];
  const int64_t waves = (int64_t)gridDim.x * (SP_T / 64);
  for (int64_t k = (int64_t)blockIdx.x * (SP_T / 64) + (threadIdx.x >> 6); k < K; k += waves) {
    const int64_t vs = cstart[k], ve = cstart[k + 1];
    const uint64_t ky = key[vs];
    const int b = (int)(ky >> 30);
    const double* gr = grid + (int64_t)b * SP_GRID;
    const double h = gr[3];
    double c[3], blo[3], bhi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double cell = (double)((ky >> (20 - 10 * a)) & 1023u);
      c[a] = gr[a] + (cell + 0.5) * h;
      blo[a] = gr[a] + cell * h;
      bhi[a] = gr[a] + (cell + 1.0) * h;
    }
    // the mean: lanes stride the cluster's vertices (ascending vertex id) from the segment's own start
    double m[3] = {0.0, 0.0, 0.0};
    for (int64_t j = vs + lane; j < ve; j += 64) {
      const int64_t g = idx[j];
#pragma unroll
      for (int a = 0; a < 3; ++a) m[a] += (double)verts[g * 3 + a];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = sp_wave_sum(m[a]) / (double)(ve - vs);
    // the quadric: lanes stride the cluster's incident faces (ascending face id)
    const int64_t is = istart[k], ie = iend[k];
    const int64_t vo = vert_off[b];
    double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0};
    for (int64_t j = is + lane; j < ie; j += 64) {
      const int64_t f = iv[j];
      double q[3][3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int64_t g = vo + faces[f * 3 + i];
#pragma unroll
        for (int a = 0; a < 3; ++a) q[i][a] = (double)verts[g * 3 + a] - c[a];
      }
      double u[3], w[3], n[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        u[a] = q[1][a] - q[0][a];
        w[a] = q[2][a] - q[0][a];
      }
      n[0] = u[1] * w[2] - u[2] * w[1];
      n[1] = u[2] * w[0] - u[0] * w[2];
      n[2] = u[0] * w[1] - u[1] * w[0];
      const double d = n[0] * q[0][0] + n[1] * q[0][1] + n[2] * q[0][2];
      A[0] += n[0] * n[0];
      A[1] += n[0] * n[1];
      A[2] += n[0] * n[2];
      A[3] += n[1] * n[1];
      A[4] += n[1] * n[2];
      A[5] += n[2] * n[2];
#pragma unroll
      for (int a = 0; a < 3; ++a) r[a] += d * n[a];
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) A[a] = sp_wave_sum(A[a]);
#pragma unroll
    for (int a = 0; a < 3; ++a) r[a] = sp_wave_sum(r[a]);
    if (lane == 0) {
      const double tr = A[0] + A[3] + A[5];
      double x[3] = {m[0], m[1], m[2]};
      if (tr != 0.0) {
        const double lam = reg * tr / 3.0;
        A[0] += lam;
        A[3] += lam;
        A[5] += lam;
#pragma unroll
        for (int a = 0; a < 3; ++a) r[a] += lam * (m[a] - c[a]);
        double y[3];
        sp_solve3(A, r, y);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const double t = y[a] + c[a];
          x[a] = t < blo[a] ? blo[a] : (t > bhi[a] ? bhi[a] : t);
        }
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) pos[k * 3 + a] = (float)x[a];
    }
  }
}

// ---- faces -----------------------------------------------------------------------------------------------------------
// the clusters of face f, rotated so that the lowest comes first (winding kept); false unless the three differ
__device__ __forceinline__ bool sp_triple(const int32_t* __restrict__ faces, const int32_t* __restrict__ cov,
                                          int64_t vo, int64_t f, uint32_t t[3]) {
  const uint32_t a = (uint32_t)cov[vo + faces[f * 3]], b = (uint32_t)cov[vo + faces[f * 3 + 1]],
                 c = (uint32_t)cov[vo + faces[f * 3 + 2]];
  if (a < b && a < c) {
    t[0] = a, t[1] = b, t[2] = c;
  } else if (b < a && b < c) {
    t[0] = b, t[1] = c, t[2] = a;
  } else {
    t[0] = c, t[1] = a, t[2] = b;
  }
  return a != b && b != c && a != c;
}

__global__ __launch_bounds__(SP_T) void sp_face_third_kernel(const int32_t* __restrict__ faces,
                                                             const int32_t* __restrict__ cov,
                                                             const int64_t* __restrict__ vert_off,
                                                             const int64_t* __restrict__ tri_off, int batch,
                                                             int64_t F, uint32_t sentinel,
                                                             int32_t* __restrict__ fflag, uint32_t* __restrict__ k32,
                                                             int32_t* __restrict__ val,
                                                             const int32_t* __restrict__ status) {
  if (status[0]) return;
  SP_LOOP(f, F) {
    uint32_t t[3];
    const bool d = sp_triple(faces, cov, vert_off[sp_shape(tri_off, batch, f)], f, t);
    fflag[f] = d;
    k32[f] = d ? t[2] : sentinel;
    val[f] = (int32_t)f;
  }
}

__global__ void sp_counts_distinct_kernel(const int32_t* __restrict__ fpre, const int64_t* __restrict__ tri_off,
                                          int batch, int64_t* __restrict__ counts,
                                          const int32_t* __restrict__ status) {
  if (status[0]) return;
  SP_LOOP(b, batch) {
    const int64_t nf = tri_off[b + 1] - tri_off[b], d = (int64_t)fpre[tri_off[b + 1]] - fpre[tri_off[b]];
    counts[b * SP_COUNTS + 3] = nf - d;
    counts[b * SP_COUNTS + 4] = d;        // minus the kept faces, once they are known
  }
}

__global__ __launch_bounds__(SP_T) void sp_face_pair_kernel(const int32_t* __restrict__ faces,
                                                            const int32_t* __restrict__ cov,
                                                            const int64_t* __restrict__ vert_off,
                                                            const int64_t* __restrict__ tri_off, int batch, int64_t F,
                                                            uint32_t sentinel, const int32_t* __restrict__ val,
                                                            uint64_t* __restrict__ k64,
                                                            const int32_t* __restrict__ status) {
  if (status[0]) return;
  SP_LOOP(i, F) {
    const int64_t f = val[i];
    uint32_t t[3];
    const bool d = sp_triple(faces, cov, vert_off[sp_shape(tri_off, batch, f)], f, t);
    k64[i] = d ? ((uint64_t)t[0] << 32) | t[1] : ((uint64_t)sentinel << 32) | sentinel;
  }
}

__global__ __launch_bounds__(SP_T) void sp_face_first_kernel(const int32_t* __restrict__ faces,
                                                             const int32_t* __restrict__ cov,
                                                             const int64_t* __restrict__ vert_off,
                                                             const int64_t* __restrict__ tri_off, int batch,
                                                             int64_t F, const int32_t* __restrict__ val,
                                                             int32_t* __restrict__ fflag,
                                                             const int32_t* __restrict__ status) {
  if (status[0]) return;
  SP_LOOP(i, F) {
    const int64_t f = val[i];
    uint32_t t[3], p[3];
    bool first = sp_triple(faces, cov, vert_off[sp_shape(tri_off, batch, f)], f, t);
    if (first && i > 0) {
      const int64_t e = val[i - 1];           // sorted before f: an earlier face if the triples are equal
      if (sp_triple(faces, cov, vert_off[sp_shape(tri_off, batch, e)], e, p))
        first = t[0] != p[0] || t[1] != p[1] || t[2] != p[2];
    }
    fflag[f] = first;
  }
}

__global__ __launch_bounds__(SP_T) void sp_used_kernel(const int32_t* __restrict__ faces,
                                                       const int32_t* __restrict__ cov,
                                                       const int32_t* __restrict__ fflag,
                                                       const int64_t* __restrict__ vert_off,
                                                       const int64_t* __restrict__ tri_off, int batch, int64_t F,
                                                       int32_t* __restrict__ used,
                                                       const int32_t* __restrict__ status) {
  if (status[0]) return;
  SP_LOOP(f, F) {
    if (!fflag[f]) continue;
    const int64_t vo = vert_off[sp_shape(tri_off, batch, f)];
#pragma unroll
    for (int j = 0; j < 3; ++j) used[cov[vo + faces[f * 3 + j]]] = 1;      // every writer stores the same value
  }
}

__global__ void sp_counts_kernel(const int32_t* __restrict__ coff, const int32_t* __restrict__ upre,
                                 const int32_t* __restrict__ fpre, const int64_t* __restrict__ tri_off, int batch,
                                 int64_t* __restrict__ counts, const int32_t* __restrict__ status) {
  if (status[0]) return;
  SP_LOOP(b, batch) {
    const int64_t kf = (int64_t)fpre[tri_off[b + 1]] - fpre[tri_off[b]];
    counts[b * SP_COUNTS] = (int64_t)coff[b + 1] - coff[b];
    counts[b * SP_COUNTS + 1] = (int64_t)upre[coff[b + 1]] - upre[coff[b]];
    counts[b * SP_COUNTS + 2] = kf;
    counts[b * SP_COUNTS + 4] -= kf;
  }
}

// ---- extract ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_T) void sp_extract_vert_kernel(const float* __restrict__ pos,
                                                               const uint64_t* __restrict__ key,
                                                               const int32_t* __restrict__ pre,
                                                               const int32_t* __restrict__ cstart,
                                                               const int32_t* __restrict__ coff,
                                                               const int32_t* __restrict__ upre, int64_t V,
                                                               const int64_t* __restrict__ new_vert_off,
                                                               float* __restrict__ out,
                                                               const int32_t* __restrict__ status) {
  if (status[0]) return;
  const int64_t K = pre[V];
  SP_LOOP(k, K) {
    if (upre[k + 1] == upre[k]) continue;
    const int b = (int)(key[cstart[k]] >> 30);
    const int64_t dst = new_vert_off[b] + (upre[k] - upre[coff[b]]);
#pragma unroll
    for (int a = 0; a < 3; ++a) out[dst * 3 + a] = pos[k * 3 + a];
  }
}

__global__ __launch_bounds__(SP_T) void sp_extract_face_kernel(const int32_t* __restrict__ faces,
                                                               const int32_t* __restrict__ cov,
                                                               const int32_t* __restrict__ coff,
                                                               const int32_t* __restrict__ upre,
                                                               const int32_t* __restrict__ fpre,
                                                               const int64_t* __restrict__ vert_off,
                                                               const int64_t* __restrict__ tri_off,
                                                               const int64_t* __restrict__ new_tri_off, int batch,
                                                               int64_t F, int32_t* __restrict__ out,
                                                               const int32_t* __restrict__ status) {
  if (status[0]) return;
  SP_LOOP(f, F) {
    if (fpre[f + 1] == fpre[f]) continue;
    const int b = sp_shape(tri_off, batch, f);
    uint32_t t[3];
    sp_triple(faces, cov, vert_off[b], f, t);
    const int64_t dst = new_tri_off[b] + (fpre[f] - fpre[tri_off[b]]);
    const int32_t base = upre[coff[b]];
#pragma unroll
    for (int j = 0; j < 3; ++j) out[dst * 3 + j] = upre[t[j]] - base;
  }
}

template <typename KeyT>
int sp_sort(const SpWs& w, const KeyT* kin, KeyT* kout, const int32_t* vin, int32_t* vout, int64_t n, int end_bit,
            hipStream_t st) {
  size_t bytes = w.sort_bytes;
  if (end_bit < 1) end_bit = 1;
  if (hipcub::DeviceRadixSort::SortPairs(w.sort_ws, bytes, kin, kout, vin, vout, (int)n, 0, end_bit, st) != hipSuccess)
    return OFX_ELAUNCH;
  return OFX_OK;
}

}  // namespace

extern "C" int ofx_simplify_stages() { return SP_STAGES; }

extern "C" size_t ofx_simplify_ws_bytes(int64_t total_verts, int64_t total_faces, int batch) {
  if (!sp_valid(total_verts, total_faces, batch)) return 0;
  return sp_layout(total_verts, total_faces, batch, nullptr, nullptr);
}

extern "C" int ofx_simplify_cluster(const float* verts, const int32_t* faces, const int64_t* vert_off,
                                    const int64_t* tri_off, int batch, int64_t total_verts, int64_t total_faces,
                                    int cells, double cell_size, double reg, int stages, int64_t* counts, void* ws,
                                    int32_t* status, void* stream) {
  const int64_t V = total_verts, F = total_faces;
  if (!sp_valid(V, F, batch) || !verts || !faces || !vert_off || !tri_off || !counts || !ws || !status)
    return OFX_EINVAL;
  if (cells < 0 || cells > SP_MAX_CELLS || !(reg > 0.0 && reg <= 1.0) || stages < 1 || stages > SP_STAGES)
    return OFX_EINVAL;
  if (cells == 0 && !(cell_size > 0.0 && cell_size <= 1.79769313486231570815e308)) return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  SpWs w;
  sp_layout(V, F, batch, (char*)ws, &w);
  const uint32_t sentinel = (uint32_t)V;           // above every cluster id
  const int vbits = sp_bits((uint64_t)V);
  int rc;

  // keys
  if (hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st) != hipSuccess) return OFX_ELAUNCH;
  if (hipMemsetAsync(counts, 0, (size_t)batch * SP_COUNTS * 8, st) != hipSuccess) return OFX_ELAUNCH;
  sp_check_kernel<<<ofx_grid(F, SP_T), SP_T, 0, st>>>(faces, vert_off, tri_off, batch, V, F, counts, status);
  sp_box_init_kernel<<<ofx_grid((int64_t)batch * 6, SP_T), SP_T, 0, st>>>(w.box, batch);
  sp_box_kernel<<<ofx_grid(ofx_cdiv(V, SP_BOX_CHUNK / 64), SP_T), SP_T, 0, st>>>(verts, vert_off, batch, V, w.box, status);
  sp_grid_kernel<<<ofx_grid(batch, SP_T), SP_T, 0, st>>>(w.box, vert_off, batch, cells, cell_size, w.grid, counts,
                                                        status);
  sp_keys_kernel<<<ofx_grid(V, SP_T), SP_T, 0, st>>>(verts, vert_off, batch, V, cells, w.grid, w.key_a, w.idx_a,
                                                    counts, status);
  OFX_LAUNCH_CHECK();
  if (stages == 1) return OFX_OK;

  // vsort
  rc = sp_sort(w, w.key_a, w.key_b, w.idx_a, w.idx_b, V, 30 + sp_bits((uint64_t)batch - 1), st);
  if (rc) return rc;
  sp_heads_kernel<<<ofx_grid(V, SP_T), SP_T, 0, st>>>(w.key_b, V, w.flag, status);
  OFX_LAUNCH_CHECK();
  rc = ofx_scan_i32(w.flag, w.pre, V, w.scan_ws, stream);
  if (rc) return rc;
  sp_ids_kernel<<<ofx_grid(V, SP_T), SP_T, 0, st>>>(w.idx_b, w.flag, w.pre, vert_off, batch, V, w.cov, w.cstart,
                                                   w.coff, status);
  OFX_LAUNCH_CHECK();
  if (stages == 2) return OFX_OK;

  // isort
  sp_incidence_kernel<<<ofx_grid(F, SP_T), SP_T, 0, st>>>(faces, w.cov, vert_off, tri_off, batch, F, sentinel, w.ik_a,
                                                         w.iv_a, status);
  OFX_LAUNCH_CHECK();
  rc = sp_sort(w, w.ik_a, w.ik_b, w.iv_a, w.iv_b, 3 * F, vbits, st);
  if (rc) return rc;
  if (hipMemsetAsync(w.istart, 0, (size_t)((char*)w.iend - (char*)w.istart) + (size_t)V * 4, st) != hipSuccess)
    return OFX_ELAUNCH;
  sp_segments_kernel<<<ofx_grid(3 * F, SP_T), SP_T, 0, st>>>(w.ik_b, 3 * F, sentinel, w.istart, w.iend, status);
  OFX_LAUNCH_CHECK();
  if (stages == 3) return OFX_OK;

  // solve
  sp_solve_kernel<<<ofx_grid(V * 64, SP_T), SP_T, 0, st>>>(verts, faces, vert_off, V, F, reg, w.grid, w.key_b, w.idx_b,
                                                          w.pre, w.cstart, w.istart, w.iend, w.iv_b, w.pos, status);
  OFX_LAUNCH_CHECK();
  if (stages == 4) return OFX_OK;

  // faces (the incidence buffers are free again)
  sp_face_third_kernel<<<ofx_grid(F, SP_T), SP_T, 0, st>>>(faces, w.cov, vert_off, tri_off, batch, F, sentinel,
                                                          w.fflag, w.ik_a, w.iv_a, status);
  OFX_LAUNCH_CHECK();
  rc = ofx_scan_i32(w.fflag, w.fpre, F, w.scan_ws, stream);
  if (rc) return rc;
  sp_counts_distinct_kernel<<<ofx_grid(batch, SP_T), SP_T, 0, st>>>(w.fpre, tri_off, batch, counts, status);
  OFX_LAUNCH_CHECK();
  rc = sp_sort(w, w.ik_a, w.ik_b, w.iv_a, w.iv_b, F, vbits, st);
  if (rc) return rc;
  sp_face_pair_kernel<<<ofx_grid(F, SP_T), SP_T, 0, st>>>(faces, w.cov, vert_off, tri_off, batch, F, sentinel, w.iv_b,
                                                         w.fk_a, status);
  OFX_LAUNCH_CHECK();
  rc = sp_sort(w, w.fk_a, w.fk_b, w.iv_b, w.iv_a, F, 32 + vbits, st);
  if (rc) return rc;
  sp_face_first_kernel<<<ofx_grid(F, SP_T), SP_T, 0, st>>>(faces, w.cov, vert_off, tri_off, batch, F, w.iv_a, w.fflag,
                                                          status);
  OFX_LAUNCH_CHECK();
  rc = ofx_scan_i32(w.fflag, w.fpre, F, w.scan_ws, stream);
  if (rc) return rc;
  if (hipMemsetAsync(w.flag, 0, (size_t)V * 4, st) != hipSuccess) return OFX_ELAUNCH;
  sp_used_kernel<<<ofx_grid(F, SP_T), SP_T, 0, st>>>(faces, w.cov, w.fflag, vert_off, tri_off, batch, F, w.flag,
                                                    status);
  OFX_LAUNCH_CHECK();
  rc = ofx_scan_i32(w.flag, w.upre, V, w.scan_ws, stream);
  if (rc) return rc;
  sp_counts_kernel<<<ofx_grid(batch, SP_T), SP_T, 0, st>>>(w.coff, w.upre, w.fpre, tri_off, batch, counts, status);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" int ofx_simplify_extract(const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off, int batch,
                                    int64_t total_verts, int64_t total_faces, const int64_t* new_vert_off,
                                    const int64_t* new_tri_off, float* out_verts, int32_t* out_faces, void* ws,
                                    const int32_t* status, void* stream) {
  const int64_t V = total_verts, F = total_faces;
  if (!sp_valid(V, F, batch) || !faces || !vert_off || !tri_off || !new_vert_off || !new_tri_off || !out_verts ||
      !out_faces || !ws || !status)
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  SpWs w;
  sp_layout(V, F, batch, (char*)ws, &w);
  sp_extract_vert_kernel<<<ofx_grid(V, SP_T), SP_T, 0, st>>>(w.pos, w.key_b, w.pre, w.cstart, w.coff, w.upre, V,
                                                            new_vert_off, out_verts, status);
  sp_extract_face_kernel<<<ofx_grid(F, SP_T), SP_T, 0, st>>>(faces, w.cov, w.coff, w.upre, w.fpre, vert_off, tri_off,
                                                            new_tri_off, batch, F, out_faces, status);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

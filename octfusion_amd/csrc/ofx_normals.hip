// Oriented normals for raw point clouds: exact k nearest neighbours inside each cloud of a ragged batch (ofx_knn), an
// unoriented PCA normal and the surface variation per point (ofx_pca_normals), and a consistent outward sign from one
// volumetric flood, a short march along +-n and a few neighbour votes (ofx_orient_normals).  octfusion_amd/normals.py
// drives the three; tests/normals_oracle.py restates every contract in numpy.  DESIGN.md 4.18.
//
// Contract (include/ofx.h):
//   distance   kn_dist2 = fma(dz, dz, fma(dy, dy, dx * dx)) from direct fp32 differences, the expression of
//              ofx_nn_search, written with explicit operations so that the compiler has no contraction to choose.  It is
//              the only place a distance is computed.
//   order      a candidate is the 64-bit key (bits(d2) << 32) | idx: d2 >= +0, so keys order as (d2, idx) does.  A row
//              is the k smallest keys of the cloud, ascending.  The k smallest elements of a set do not depend on the
//              order they were offered in: the counting sort below places the points of a cell in the order its
//              atomics resolved, and the result is still bitwise the same for every grid, alone or in a batch.
//   search     each cloud is binned in c^3 cells of its bounding cube (count -> ofx_scan_i32 -> fill: sorted [total]
//              float4 = x, y, z, bits(idx)).  A query visits the cells of Chebyshev shell r = 0, 1, ... around its own
//              cell, rows of x-adjacent cells as one contiguous range, and stops once the list is full and its k-th
//              distance lies below the squared distance to the nearest face of the searched block of cells that still
//              has cells behind it, less a slack of 2^-18 of the cube's side: the cell of a coordinate is a monotone
//              function of it (a subtraction of a constant, a product with a positive constant, floor, clamp), so a
//              point filed in a cell beyond a face cannot lie on the near side of it by more than the rounding of those
//              three operations, 2^-21 of the side.  c = 1 is the brute-force sweep.
//   selection  one query per lane, lanes in sorted order (neighbouring lanes ask neighbouring cells); the k-best list
//              lives in LDS as list[j][lane], 8 * k bytes per lane (32 KiB per 64-lane block at k = 64), with the
//              current k-th key in a register: a candidate that does not beat it costs no LDS access.  No scratch.
//   PCA        fp64 centroid and covariance in neighbour order, cyclic Jacobi with PN_SWEEPS fixed sweeps.
//   orient     bit grids of (G + 2)^3 cells per cloud, 32 x-cells per word.  Occupancy by atomicOr of a point's cell
//              and its six neighbours; the exterior flood runs in one block per cloud, sweeping its words in place
//              until a sweep changes nothing (the set only grows and every word has one writer, so the fixed point
//              does not depend on the schedule; a word is filled along x in registers, so information crosses 32
//              cells per sweep in x and one in y, z).  March and votes are one thread per point.
#include "ofx_common.h"

#include <cmath>

namespace {

constexpr int KN_T = 64;              // queries per block: one wave, one query per lane
constexpr int KN_MAXK = 64;
constexpr int KN_MAXC = 128;          // largest forced grid
constexpr int KN_AUTO_MAXC = 64;      // largest automatic grid
constexpr int KN_PER_CELL2 = 32;      // automatic rule: c = floor(sqrt(n / 32)), surface samples fill ~4 c^2 cells
constexpr uint64_t KN_NONE = ((uint64_t)0x7f800000u << 32) | 0xffffffffu;     // d2 = +inf, idx = -1
constexpr int PN_T = 256;
constexpr int PN_SWEEPS = 8;
constexpr int OR_FLOOD_T = 1024;
constexpr int OR_MIN_G = 8, OR_MAX_G = 128, OR_MAX_STEPS = 64, OR_MAX_ROUNDS = 64;

struct KnCloud {
  float lo[3];
  float h, inv_h, slack;
  int c, pad;
};

__host__ __device__ inline int kn_auto_cells(int64_t n) {
  int c = 1;
  while (c < KN_AUTO_MAXC && (int64_t)(c + 1) * (c + 1) * KN_PER_CELL2 <= n) ++c;
  return c;
}

__device__ __forceinline__ float kn_dist2(float qx, float qy, float qz, float tx, float ty, float tz) {
  const float dx = __fsub_rn(qx, tx), dy = __fsub_rn(qy, ty), dz = __fsub_rn(qz, tz);
  return __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, __fmul_rn(dx, dx)));
}

// monotone in x; NaN and anything below the cube land in cell 0, anything above in cell c - 1
__device__ __forceinline__ int kn_cell(float x, float lo, float inv_h, int c) {
  const float v = floorf(__fmul_rn(__fsub_rn(x, lo), inv_h));
  return (int)fminf(fmaxf(v, 0.f), (float)(c - 1));
}

// one block per cloud: the bounding cube and the grid of the cloud
__global__ __launch_bounds__(PN_T) void kn_bbox_kernel(const float* __restrict__ p, const int64_t* __restrict__ off,
                                                       int cells, int cmax, KnCloud* __restrict__ clouds) {
  __shared__ float red[6][PN_T];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t base = off[b], n = off[b + 1] - base;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = tid; i < n; i += PN_T)
    for (int a = 0; a < 3; ++a) {
      const float v = p[(base + i) * 3 + a];
      mn[a] = fminf(mn[a], v);
      mx[a] = fmaxf(mx[a], v);
    }
  for (int a = 0; a < 3; ++a) {
    red[a][tid] = mn[a];
    red[3 + a][tid] = mx[a];
  }
  __syncthreads();
  for (int s = PN_T / 2; s > 0; s >>= 1) {
    if (tid < s)
      for (int a = 0; a < 3; ++a) {
        red[a][tid] = fminf(red[a][tid], red[a][tid + s]);
        red[3 + a][tid] = fmaxf(red[3 + a][tid], red[3 + a][tid + s]);
      }
    __syncthreads();
  }
  if (tid == 0) {
    KnCloud g;
    float e = 0.f;
    for (int a = 0; a < 3; ++a) e = fmaxf(e, red[3 + a][0] - red[a][0]);
    int c = cells > 0 ? cells : kn_auto_cells(n);
    if (c > cmax) c = cmax;
    if (!(e > 0.f) || !(e < INFINITY) || n < 1) {      // one point, identical points, non-finite input: one cell
      c = 1;
      e = 1.f;
      for (int a = 0; a < 3; ++a) g.lo[a] = 0.f;
    } else {
      for (int a = 0; a < 3; ++a) g.lo[a] = (red[a][0] + red[3 + a][0]) * 0.5f - e * 0.5f;
    }
    g.c = c;
    g.h = e / (float)c;
    g.inv_h = (float)c / e;
    g.slack = e * 0x1p-18f;
    g.pad = 0;
    clouds[b] = g;
  }
}

// grid (chunks, batch): cell of every point, and the population of every cell
__global__ __launch_bounds__(PN_T) void kn_count_kernel(const float* __restrict__ p, const int64_t* __restrict__ off,
                                                        const KnCloud* __restrict__ clouds, int64_t cstride,
                                                        int32_t* __restrict__ cellid, int32_t* __restrict__ cnt) {
  const int b = blockIdx.y;
  const int64_t base = off[b], n = off[b + 1] - base;
  const KnCloud g = clouds[b];
  for (int64_t i = (int64_t)blockIdx.x * PN_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PN_T) {
    const float* s = p + (base + i) * 3;
    const int cx = kn_cell(s[0], g.lo[0], g.inv_h, g.c), cy = kn_cell(s[1], g.lo[1], g.inv_h, g.c),
              cz = kn_cell(s[2], g.lo[2], g.inv_h, g.c);
    const int32_t cell = (int32_t)(b * cstride + ((int64_t)cz * g.c + cy) * g.c + cx);
    cellid[base + i] = cell;
    atomicAdd(cnt + cell, 1);
  }
}

// the slot inside a cell is whatever the atomic hands out: see 'order' above
__global__ __launch_bounds__(PN_T) void kn_fill_kernel(const float* __restrict__ p, const int64_t* __restrict__ off,
                                                       const int32_t* __restrict__ cellid,
                                                       const int32_t* __restrict__ start, int32_t* __restrict__ cursor,
                                                       float4* __restrict__ sorted) {
  const int b = blockIdx.y;
  const int64_t base = off[b], n = off[b + 1] - base;
  for (int64_t i = (int64_t)blockIdx.x * PN_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PN_T) {
    const float* s = p + (base + i) * 3;
    const int32_t cell = cellid[base + i];
    const int32_t pos = start[cell] + atomicAdd(cursor + cell, 1);
    sorted[pos] = make_float4(s[0], s[1], s[2], __int_as_float((int32_t)i));
  }
}

__device__ __forceinline__ void kn_scan_range(const float4* __restrict__ sorted, int32_t t0, int32_t t1, float qx,
                                              float qy, float qz, uint64_t* L, int k, uint64_t& worst) {
  for (int32_t t = t0; t < t1; ++t) {
    const float4 s = sorted[t];
    const float d = kn_dist2(qx, qy, qz, s.x, s.y, s.z);
    const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)__float_as_int(s.w);
    if (key < worst) {                       // beats the current k-th: shift the tail up and drop it in
      int j = k - 1;
      while (j > 0) {
        const uint64_t prev = L[(j - 1) * KN_T];
        if (prev <= key) break;
        L[j * KN_T] = prev;
        --j;
      }
      L[j * KN_T] = key;
      worst = L[(k - 1) * KN_T];
    }
  }
}

// grid (chunks of KN_T sorted positions, batch); dynamic LDS: k * KN_T keys
__global__ __launch_bounds__(KN_T) void kn_query_kernel(const float4* __restrict__ sorted,
                                                        const int32_t* __restrict__ start,
                                                        const KnCloud* __restrict__ clouds,
                                                        const int64_t* __restrict__ off, int k, int64_t cstride,
                                                        int32_t* __restrict__ idx, float* __restrict__ d2) {
  extern __shared__ uint64_t kn_list[];
  const int b = blockIdx.y;
  const int64_t base = off[b], n = off[b + 1] - base;
  const int64_t s = (int64_t)blockIdx.x * KN_T + threadIdx.x;
  if (s >= n) return;
  uint64_t* L = kn_list + threadIdx.x;
  for (int j = 0; j < k; ++j) L[j * KN_T] = KN_NONE;
  uint64_t worst = KN_NONE;
  const KnCloud g = clouds[b];
  const int c = g.c;
  const int32_t* st = start + b * cstride;
  const float4 q = sorted[base + s];
  const int cx = kn_cell(q.x, g.lo[0], g.inv_h, c), cy = kn_cell(q.y, g.lo[1], g.inv_h, c),
            cz = kn_cell(q.z, g.lo[2], g.inv_h, c);
  const float rx = __fsub_rn(q.x, g.lo[0]), ry = __fsub_rn(q.y, g.lo[1]), rz = __fsub_rn(q.z, g.lo[2]);
  for (int r = 0; r < c; ++r) {
    const int x0 = max(cx - r, 0), x1 = min(cx + r, c - 1);
    const int y0 = max(cy - r, 0), y1 = min(cy + r, c - 1);
    const int z0 = max(cz - r, 0), z1 = min(cz + r, c - 1);
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const int32_t* row = st + ((int64_t)z * c + y) * c;
        if (z - cz == r || cz - z == r || y - cy == r || cy - y == r) {
          kn_scan_range(sorted, row[x0], row[x1 + 1], q.x, q.y, q.z, L, k, worst);
        } else {
          if (cx - r >= 0) kn_scan_range(sorted, row[cx - r], row[cx - r + 1], q.x, q.y, q.z, L, k, worst);
          if (cx + r <= c - 1) kn_scan_range(sorted, row[cx + r], row[cx + r + 1], q.x, q.y, q.z, L, k, worst);
        }
      }
    if (x0 == 0 && y0 == 0 && z0 == 0 && x1 == c - 1 && y1 == c - 1 && z1 == c - 1) break;   // the whole cloud
    if (worst == KN_NONE) continue;
    float gap = INFINITY;
    if (x0 > 0) gap = fminf(gap, rx - (float)x0 * g.h);
    if (y0 > 0) gap = fminf(gap, ry - (float)y0 * g.h);
    if (z0 > 0) gap = fminf(gap, rz - (float)z0 * g.h);
    if (x1 < c - 1) gap = fminf(gap, (float)(x1 + 1) * g.h - rx);
    if (y1 < c - 1) gap = fminf(gap, (float)(y1 + 1) * g.h - ry);
    if (z1 < c - 1) gap = fminf(gap, (float)(z1 + 1) * g.h - rz);
    gap -= g.slack;
    if (gap > 0.f && __uint_as_float((uint32_t)(worst >> 32)) < gap * gap * (1.f - 0x1p-18f)) break;
  }
  const int64_t row = (base + (int64_t)__float_as_int(q.w)) * k;
  for (int j = 0; j < k; ++j) {
    const uint64_t key = L[j * KN_T];
    idx[row + j] = (int32_t)(uint32_t)key;
    d2[row + j] = __uint_as_float((uint32_t)(key >> 32));
  }
}

// ------------------------------------------------------------------------------------------------------------ PCA
// one Jacobi rotation of the symmetric 3x3 (p, q; r the third index) and of the eigenvector columns p, q
__device__ __forceinline__ void pn_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                          double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  double a = arp, bq = arq;
  arp = c * a - s * bq;
  arq = s * a + c * bq;
  a = v0p, bq = v0q;
  v0p = c * a - s * bq;
  v0q = s * a + c * bq;
  a = v1p, bq = v1q;
  v1p = c * a - s * bq;
  v1q = s * a + c * bq;
  a = v2p, bq = v2q;
  v2p = c * a - s * bq;
  v2q = s * a + c * bq;
}

__global__ __launch_bounds__(PN_T) void pn_pca_kernel(const float* __restrict__ p, const int64_t* __restrict__ off,
                                                      const int32_t* __restrict__ idx, int k,
                                                      float* __restrict__ normals, float* __restrict__ variation,
                                                      int32_t* __restrict__ degenerate) {
  const int b = blockIdx.y;
  const int64_t base = off[b], n = off[b + 1] - base;
  for (int64_t i = (int64_t)blockIdx.x * PN_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PN_T) {
    const int32_t* nb = idx + (base + i) * k;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    int m = 0;
    for (int j = 0; j < k; ++j) {
      const int32_t t = nb[j];
      if (t < 0 || t >= n) continue;
      const float* s = p + (base + t) * 3;
      sx += (double)s[0];
      sy += (double)s[1];
      sz += (double)s[2];
      ++m;
    }
    float out[3] = {0.f, 0.f, 0.f}, var = 0.f;
    bool ok = m >= 3;
    if (ok) {
      const double cx = sx / m, cy = sy / m, cz = sz / m;
      double a00 = 0.0, a11 = 0.0, a22 = 0.0, a01 = 0.0, a02 = 0.0, a12 = 0.0;
      for (int j = 0; j < k; ++j) {
        const int32_t t = nb[j];
        if (t < 0 || t >= n) continue;
        const float* s = p + (base + t) * 3;
        const double dx = (double)s[0] - cx, dy = (double)s[1] - cy, dz = (double)s[2] - cz;
        a00 += dx * dx;
        a11 += dy * dy;
        a22 += dz * dz;
        a01 += dx * dy;
        a02 += dx * dz;
        a12 += dy * dz;
      }
      a00 /= m, a11 /= m, a22 /= m, a01 /= m, a02 /= m, a12 /= m;
      double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll 1
      for (int sweep = 0; sweep < PN_SWEEPS; ++sweep) {
        pn_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        pn_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        pn_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
      }
      const double sum = a00 + a11 + a22;
      ok = sum > 0.0;
      if (ok) {
        const bool s1 = a11 < a00;                     // the smallest eigenvalue, lowest index on ties
        double l = s1 ? a11 : a00, ex = s1 ? v01 : v00, ey = s1 ? v11 : v10, ez = s1 ? v21 : v20;
        const bool s2 = a22 < l;
        l = s2 ? a22 : l, ex = s2 ? v02 : ex, ey = s2 ? v12 : ey, ez = s2 ? v22 : ez;
        const double len = sqrt(ex * ex + ey * ey + ez * ez);
        out[0] = (float)(ex / len);
        out[1] = (float)(ey / len);
        out[2] = (float)(ez / len);
        const float m0 = fabsf(out[0]), m1 = fabsf(out[1]), m2 = fabsf(out[2]);
        const float lead = m2 > fmaxf(m0, m1) ? out[2] : (m1 > m0 ? out[1] : out[0]);      // lowest axis on ties
        if (lead < 0.f) out[0] = -out[0], out[1] = -out[1], out[2] = -out[2];
        var = (float)((l > 0.0 ? l : 0.0) / sum);
      }
    }
    if (!ok) atomicAdd(degenerate + b, 1);
    normals[(base + i) * 3 + 0] = out[0];
    normals[(base + i) * 3 + 1] = out[1];
    normals[(base + i) * 3 + 2] = out[2];
    variation[base + i] = var;
  }
}

// --------------------------------------------------------------------------------------------------------- orient
struct OrGrid {
  float lo[3], h;
  int G, D, W;          // cells per axis, D = G + 2 with the border layer, W words per x-row
};

__device__ __forceinline__ OrGrid or_grid(const float* lo, const float* e, const int32_t* g, int b, int max_g) {
  OrGrid r;
  r.G = min(max(g[b], 1), max_g);            // the caller keeps 8 <= G <= max_g; never index past the workspace
  r.D = r.G + 2;
  r.W = (r.D + 31) >> 5;
  r.lo[0] = lo[b * 3 + 0];
  r.lo[1] = lo[b * 3 + 1];
  r.lo[2] = lo[b * 3 + 2];
  r.h = __fdiv_rn(e[b], (float)r.G);
  return r;
}

__device__ __forceinline__ float or_coord(float x, float lo, float h) {
  return floorf(__fdiv_rn(__fsub_rn(x, lo), h));
}

__device__ __forceinline__ int64_t or_word(const OrGrid& g, int x, int y, int z) {
  return ((int64_t)z * g.D + y) * g.W + (x >> 5);
}

__global__ __launch_bounds__(PN_T) void or_mark_kernel(const float* __restrict__ p, const int64_t* __restrict__ off,
                                                       const float* __restrict__ lo, const float* __restrict__ e,
                                                       const int32_t* __restrict__ gs, int max_g, int64_t wstride,
                                                       uint32_t* __restrict__ occ) {
  const int b = blockIdx.y;
  const int64_t base = off[b], n = off[b + 1] - base;
  const OrGrid g = or_grid(lo, e, gs, b, max_g);
  uint32_t* o = occ + b * wstride;
  for (int64_t i = (int64_t)blockIdx.x * PN_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PN_T) {
    const float* s = p + (base + i) * 3;
    int c[3];
    for (int a = 0; a < 3; ++a)
      c[a] = (int)fminf(fmaxf(or_coord(s[a], g.lo[a], g.h), 0.f), (float)(g.G - 1)) + 1;      // in [1, G]
    atomicOr(o + or_word(g, c[0], c[1], c[2]), 1u << (c[0] & 31));
    atomicOr(o + or_word(g, c[0] - 1, c[1], c[2]), 1u << ((c[0] - 1) & 31));
    atomicOr(o + or_word(g, c[0] + 1, c[1], c[2]), 1u << ((c[0] + 1) & 31));
    atomicOr(o + or_word(g, c[0], c[1] - 1, c[2]), 1u << (c[0] & 31));
    atomicOr(o + or_word(g, c[0], c[1] + 1, c[2]), 1u << (c[0] & 31));
    atomicOr(o + or_word(g, c[0], c[1], c[2] - 1), 1u << (c[0] & 31));
    atomicOr(o + or_word(g, c[0], c[1], c[2] + 1), 1u << (c[0] & 31));
  }
}

__device__ __forceinline__ uint32_t or_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one block per cloud; ext is zero on entry
__global__ __launch_bounds__(OR_FLOOD_T) void or_flood_kernel(const uint32_t* __restrict__ occ_all,
                                                              uint32_t* __restrict__ ext_all,
                                                              const int32_t* __restrict__ gs, int max_g,
                                                              int64_t wstride) {
  __shared__ int changed;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int G = min(max(gs[b], 1), max_g), D = G + 2, W = (D + 31) >> 5;
  const int nw = D * D * W;
  const uint32_t* occ = occ_all + b * wstride;
  uint32_t* ext = ext_all + b * wstride;
  const uint32_t last_valid = (D & 31) ? ((1u << (D & 31)) - 1u) : 0xffffffffu;
  for (int w = tid; w < nw; w += OR_FLOOD_T) {          // seeds: the border layer, where it is not occupied
    const int xw = w % W, y = (w / W) % D, z = w / (W * D);
    const uint32_t valid = xw == W - 1 ? last_valid : 0xffffffffu;
    uint32_t border = 0;
    if (z == 0 || z == D - 1 || y == 0 || y == D - 1) border = valid;
    if (xw == 0) border |= 1u;
    if (xw == (D - 1) >> 5) border |= 1u << ((D - 1) & 31);
    __hip_atomic_store(ext + w, border & valid & ~occ[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  for (int64_t sweep = 0; sweep < (int64_t)D * D * D + 1; ++sweep) {      // every sweep but the last adds a cell
    if (tid == 0) changed = 0;
    __syncthreads();
    bool mine = false;
    for (int w = tid; w < nw; w += OR_FLOOD_T) {
      const int xw = w % W, y = (w / W) % D, z = w / (W * D);
      const uint32_t valid = xw == W - 1 ? last_valid : 0xffffffffu;
      const uint32_t free_ = ~occ[w] & valid;
      const uint32_t cur = or_load(ext + w);
      uint32_t s = cur;
      if (y > 0) s |= or_load(ext + w - W);
      if (y < D - 1) s |= or_load(ext + w + W);
      if (z > 0) s |= or_load(ext + w - W * D);
      if (z < D - 1) s |= or_load(ext + w + W * D);
      if (xw > 0) s |= or_load(ext + w - 1) >> 31;
      if (xw < W - 1) s |= or_load(ext + w + 1) << 31;
      s &= free_;
      for (;;) {                                         // along x inside the word
        const uint32_t t = (s | (s << 1) | (s >> 1)) & free_;
        if (t == s) break;
        s = t;
      }
      if (s != cur) {
        __hip_atomic_store(ext + w, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        mine = true;
      }
    }
    if (mine) changed = 1;
    __syncthreads();
    const int again = changed;
    __syncthreads();
    if (!again) break;
  }
}

// first half-cell step s in 1..2S at which p + s (h/2) d sits in an exterior cell or outside the array; 2S + 1: none
__device__ __forceinline__ int or_first_exit(const OrGrid& g, const uint32_t* __restrict__ ext, const float* s,
                                             float dx, float dy, float dz, int steps2) {
  const float h2 = __fmul_rn(g.h, 0.5f);
  for (int k = 1; k <= steps2; ++k) {
    const float t = __fmul_rn((float)k, h2);
    const float qx = __fadd_rn(s[0], __fmul_rn(t, dx)), qy = __fadd_rn(s[1], __fmul_rn(t, dy)),
                qz = __fadd_rn(s[2], __fmul_rn(t, dz));
    const float vx = or_coord(qx, g.lo[0], g.h), vy = or_coord(qy, g.lo[1], g.h), vz = or_coord(qz, g.lo[2], g.h);
    const float top = (float)g.G;
    if (!(vx >= -1.f && vx <= top && vy >= -1.f && vy <= top && vz >= -1.f && vz <= top)) return k;   // NaN: outside
    const int x = (int)vx + 1, y = (int)vy + 1, z = (int)vz + 1;
    if ((ext[or_word(g, x, y, z)] >> (x & 31)) & 1u) return k;
  }
  return steps2 + 1;
}

// counts [batch, 4]: undecided_after_march, flipped_by_vote, undecided, degenerate
__global__ __launch_bounds__(PN_T) void or_march_kernel(const float* __restrict__ p, const float* __restrict__ nrm,
                                                        const int64_t* __restrict__ off, const float* __restrict__ lo,
                                                        const float* __restrict__ e, const int32_t* __restrict__ gs,
                                                        int max_g, int64_t wstride, const uint32_t* __restrict__ ext,
                                                        int steps2, int8_t* __restrict__ sign,
                                                        int32_t* __restrict__ counts) {
  const int b = blockIdx.y;
  const int64_t base = off[b], n = off[b + 1] - base;
  const OrGrid g = or_grid(lo, e, gs, b, max_g);
  const uint32_t* x = ext + b * wstride;
  for (int64_t i = (int64_t)blockIdx.x * PN_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PN_T) {
    const float* s = p + (base + i) * 3;
    const float* d = nrm + (base + i) * 3;
    const int fa = or_first_exit(g, x, s, d[0], d[1], d[2], steps2);
    const int fb = or_first_exit(g, x, s, -d[0], -d[1], -d[2], steps2);
    const int8_t sg = fa < fb ? 1 : (fb < fa ? -1 : 0);
    sign[base + i] = sg;
    if (sg == 0) atomicAdd(counts + b * 4 + 0, 1);
    if (d[0] == 0.f && d[1] == 0.f && d[2] == 0.f) atomicAdd(counts + b * 4 + 3, 1);
  }
}

__global__ __launch_bounds__(PN_T) void or_vote_kernel(const float* __restrict__ nrm, const int64_t* __restrict__ off,
                                                       const int32_t* __restrict__ idx, int k,
                                                       const int8_t* __restrict__ in, int8_t* __restrict__ out) {
  const int b = blockIdx.y;
  const int64_t base = off[b], n = off[b + 1] - base;
  for (int64_t i = (int64_t)blockIdx.x * PN_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PN_T) {
    const float* a = nrm + (base + i) * 3;
    const double ax = a[0], ay = a[1], az = a[2];
    const int32_t* nb = idx + (base + i) * k;
    double d = 0.0;
    for (int j = 0; j < k; ++j) {
      const int32_t t = nb[j];
      if (t < 0 || t >= n) continue;
      const float* c = nrm + (base + t) * 3;
      const double dot = ((double)c[0] * ax + (double)c[1] * ay) + (double)c[2] * az;
      d += (double)in[base + t] * dot;
    }
    out[base + i] = d > 0.0 ? (int8_t)1 : (d < 0.0 ? (int8_t)-1 : in[base + i]);
  }
}

__global__ __launch_bounds__(PN_T) void or_final_kernel(const float* __restrict__ nrm, const int64_t* __restrict__ off,
                                                        const int8_t* __restrict__ marched,
                                                        const int8_t* __restrict__ voted, float* __restrict__ out,
                                                        int8_t* __restrict__ sign, int32_t* __restrict__ counts) {
  const int b = blockIdx.y;
  const int64_t base = off[b], n = off[b + 1] - base;
  for (int64_t i = (int64_t)blockIdx.x * PN_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * PN_T) {
    const int8_t m = marched[base + i], v = voted[base + i];
    const float f = v < 0 ? -1.f : 1.f;
    for (int a = 0; a < 3; ++a) {
      const float c = nrm[(base + i) * 3 + a];
      out[(base + i) * 3 + a] = f < 0.f ? -c : c;
    }
    if (sign) sign[base + i] = v;
    if (m != 0 && v == -m) atomicAdd(counts + b * 4 + 1, 1);
    if (v == 0) atomicAdd(counts + b * 4 + 2, 1);
  }
}

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

struct KnWs {
  KnCloud* clouds;
  int32_t *cnt, *start, *cellid;
  float4* sorted;
  void* scan_ws;
  size_t bytes;
};

KnWs kn_layout(void* ws, int batch, int64_t total, int64_t ncell) {
  KnWs l;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    void* r = ws ? (char*)ws + at : nullptr;
    at += al256(bytes);
    return r;
  };
  l.clouds = (KnCloud*)take((size_t)batch * sizeof(KnCloud));
  l.cnt = (int32_t*)take((size_t)ncell * 4);
  l.start = (int32_t*)take((size_t)(ncell + 1) * 4);
  l.cellid = (int32_t*)take((size_t)total * 4);
  l.sorted = (float4*)take((size_t)total * sizeof(float4));
  l.scan_ws = take(ofx_scan_ws_bytes(ncell));
  l.bytes = at;
  return l;
}

// cells per axis the workspace is laid out for, 0 for arguments out of range
int kn_cmax(int batch, int64_t total, int64_t max_n, int cells) {
  if (batch < 1 || batch > 65535 || total < 1 || total > INT32_MAX || max_n < 1 || max_n > total || cells < 0 ||
      cells > KN_MAXC)
    return 0;
  const int c = cells > 0 ? cells : kn_auto_cells(max_n);
  if ((int64_t)batch * c * c * c > INT32_MAX / 2) return 0;
  return c;
}

struct OrWs {
  uint32_t *occ, *ext;
  int8_t *s0, *sa, *sb;
  int64_t wstride;
  size_t bits_bytes, bytes;
};

OrWs or_layout(void* ws, int batch, int64_t total, int max_g) {
  OrWs l;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    void* r = ws ? (char*)ws + at : nullptr;
    at += al256(bytes);
    return r;
  };
  const int64_t D = max_g + 2;
  l.wstride = D * D * ((D + 31) / 32);
  l.bits_bytes = al256((size_t)batch * l.wstride * 4);
  l.occ = (uint32_t*)take(l.bits_bytes);          // occ and ext are adjacent: one memset clears both
  l.ext = (uint32_t*)take(l.bits_bytes);
  l.s0 = (int8_t*)take((size_t)total);
  l.sa = (int8_t*)take((size_t)total);
  l.sb = (int8_t*)take((size_t)total);
  l.bytes = at;
  return l;
}

inline dim3 pn_grid(int64_t max_n, int batch) {
  int64_t g = ofx_cdiv(max_n, PN_T);
  if (g > 1024) g = 1024;
  return dim3((unsigned)g, (unsigned)batch);
}

}  // namespace

extern "C" int ofx_knn_cells(int64_t n) { return n < 1 ? 1 : kn_auto_cells(n); }

extern "C" size_t ofx_knn_ws_bytes(int batch, int64_t total, int64_t max_n, int cells) {
  const int c = kn_cmax(batch, total, max_n, cells);
  if (!c) return 0;
  return kn_layout(nullptr, batch, total, (int64_t)batch * c * c * c).bytes;
}

extern "C" int ofx_knn(const float* p, const int64_t* off, int batch, int64_t total, int64_t max_n, int k, int cells,
                       void* ws, int32_t* idx, float* d2, void* stream) {
  if (batch < 0 || total < 0 || max_n < 0 || k < 1 || k > KN_MAXK || cells < 0) return OFX_EINVAL;
  if (batch == 0 || total == 0) return OFX_OK;
  const int c = kn_cmax(batch, total, max_n, cells);
  if (!c || !p || !off || !ws || !idx || !d2 || ofx_cdiv(max_n, KN_T) > INT32_MAX) return OFX_EINVAL;
  const int64_t cstride = (int64_t)c * c * c, ncell = batch * cstride;
  const KnWs w = kn_layout(ws, batch, total, ncell);
  hipStream_t st = ofx_stream(stream);
  kn_bbox_kernel<<<batch, PN_T, 0, st>>>(p, off, cells, c, w.clouds);
  OFX_LAUNCH_CHECK();
  if (hipMemsetAsync(w.cnt, 0, (size_t)ncell * 4, st) != hipSuccess) return OFX_ELAUNCH;
  kn_count_kernel<<<pn_grid(max_n, batch), PN_T, 0, st>>>(p, off, w.clouds, cstride, w.cellid, w.cnt);
  OFX_LAUNCH_CHECK();
  const int rc = ofx_scan_i32(w.cnt, w.start, ncell, w.scan_ws, stream);
  if (rc != OFX_OK) return rc;
  if (hipMemsetAsync(w.cnt, 0, (size_t)ncell * 4, st) != hipSuccess) return OFX_ELAUNCH;
  kn_fill_kernel<<<pn_grid(max_n, batch), PN_T, 0, st>>>(p, off, w.cellid, w.start, w.cnt, w.sorted);
  OFX_LAUNCH_CHECK();
  kn_query_kernel<<<dim3((unsigned)ofx_cdiv(max_n, KN_T), (unsigned)batch), KN_T, (size_t)k * KN_T * sizeof(uint64_t),
                    st>>>(w.sorted, w.start, w.clouds, off, k, cstride, idx, d2);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" int ofx_pca_normals(const float* p, const int64_t* off, const int32_t* idx, int batch, int64_t total,
                               int64_t max_n, int k, float* normals, float* variation, int32_t* degenerate,
                               void* stream) {
  if (batch < 0 || total < 0 || max_n < 0 || k < 1 || k > KN_MAXK) return OFX_EINVAL;
  if (batch == 0 || total == 0) return OFX_OK;
  if (!p || !off || !idx || !normals || !variation || !degenerate || batch > 65535 || total > INT32_MAX || max_n < 1 ||
      max_n > total)
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  if (hipMemsetAsync(degenerate, 0, (size_t)batch * 4, st) != hipSuccess) return OFX_ELAUNCH;
  pn_pca_kernel<<<pn_grid(max_n, batch), PN_T, 0, st>>>(p, off, idx, k, normals, variation, degenerate);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" size_t ofx_orient_normals_ws_bytes(int batch, int64_t total, int max_g) {
  if (batch < 1 || batch > 65535 || total < 1 || max_g < OR_MIN_G || max_g > OR_MAX_G) return 0;
  return or_layout(nullptr, batch, total, max_g).bytes;
}

extern "C" int ofx_orient_normals(const float* p, const float* n, const int64_t* off, const int32_t* idx, int batch,
                                  int64_t total, int64_t max_n, int k, const float* lo, const float* e,
                                  const int32_t* g, int max_g, int steps, int rounds, void* ws, float* out,
                                  int8_t* sign, int32_t* counts, void* stream) {
  if (batch < 0 || total < 0 || max_n < 0 || k < 1 || k > KN_MAXK || steps < 1 || steps > OR_MAX_STEPS ||
      rounds < 0 || rounds > OR_MAX_ROUNDS || max_g < OR_MIN_G || max_g > OR_MAX_G)
    return OFX_EINVAL;
  if (batch == 0 || total == 0) return OFX_OK;
  if (!p || !n || !off || !idx || !lo || !e || !g || !ws || !out || !counts || batch > 65535 || total > INT32_MAX ||
      max_n < 1 ||
      max_n > total)
    return OFX_EINVAL;
  const OrWs w = or_layout(ws, batch, total, max_g);
  hipStream_t st = ofx_stream(stream);
  if (hipMemsetAsync(w.occ, 0, 2 * w.bits_bytes, st) != hipSuccess) return OFX_ELAUNCH;
  if (hipMemsetAsync(counts, 0, (size_t)batch * 16, st) != hipSuccess) return OFX_ELAUNCH;
  const dim3 grid = pn_grid(max_n, batch);
  or_mark_kernel<<<grid, PN_T, 0, st>>>(p, off, lo, e, g, max_g, w.wstride, w.occ);
  OFX_LAUNCH_CHECK();
  or_flood_kernel<<<batch, OR_FLOOD_T, 0, st>>>(w.occ, w.ext, g, max_g, w.wstride);
  OFX_LAUNCH_CHECK();
  or_march_kernel<<<grid, PN_T, 0, st>>>(p, n, off, lo, e, g, max_g, w.wstride, w.ext, 2 * steps, w.s0, counts);
  OFX_LAUNCH_CHECK();
  const int8_t* cur = w.s0;
  for (int r = 0; r < rounds; ++r) {
    int8_t* nxt = (r & 1) ? w.sb : w.sa;
    or_vote_kernel<<<grid, PN_T, 0, st>>>(n, off, idx, k, cur, nxt);
    OFX_LAUNCH_CHECK();
    cur = nxt;
  }
  or_final_kernel<<<grid, PN_T, 0, st>>>(n, off, w.s0, cur, out, sign, counts);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

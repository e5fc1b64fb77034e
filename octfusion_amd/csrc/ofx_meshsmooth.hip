// The mesh as a graph, and the two things done with it: fairing (Laplacian / Taubin) and per-vertex normals.
// Contract: include/ofx.h; tests/smooth_oracle.py restates it in numpy float64.  DESIGN.md section 4.23 has the reasons
// and the figures.
//
//   adjacency  the 6 F directed pairs (vertex, neighbour) of the faces that take part, keyed vertex << 31 | neighbour in
//              indices of the whole call, the pair's own number 6 face + 2 corner + side in the payload; ONE stable sort
//              (ofx_points_sort).  A run of equal keys is one edge seen from one end, as long as the edge has faces, and
//              the sort being stable it lists those faces in the order of the vertex's corners.  Head flags, one scan:
//              the heads are the compacted neighbour rows; row_off by a binary search per vertex; the flags of a vertex
//              from the run lengths of its own row.  The vertex-to-corner index: a second sort, of the 3 F corners by
//              their vertex.
//   normals    one lane per vertex walks its corners in that order and adds the face terms in fp64.
//   smooth     fp64 state in two buffers of the workspace; weights and the rule of every vertex fixed once; then one
//              launch per half-step, a gather through the rows (one lane per vertex, a loop over its row) from one
//              buffer into the other.  Rounded to fp32 once, at the end.
// No atomics at all: every sum has the order the contract gives it.
#pragma clang fp contract(off)

#include "ofx_meshtopo.h"

namespace {

constexpr int64_t SM_MAX_F = (int64_t(1) << 30) / 6;       // 6 F pairs in one ofx_points_sort
constexpr int SM_MAX_ITERS = 10000;

bool sm_args_ok(int batch, int64_t V, int64_t F) {
  return batch >= 1 && batch <= 65535 && V >= 1 && V <= MC_MAX_V && F >= 1 && F <= SM_MAX_F;
}

// rule of a vertex in a half-step
enum { SM_REFUSED = -1, SM_PINNED = 0, SM_MOVES = 1, SM_SLIDES = 2 };

struct AdjWs {
  TbBins bins;
  McSort sort;                    // 6 F pairs, or 3 F corners
  int32_t *flag, *scan;           // [6 F], [6 F + 1]
  void* scan_ws;
  int32_t* run;                   // [6 F + 1] where the run of neighbour slot r begins in the sorted pairs
};
size_t adj_layout(int batch, int64_t F, Carver& c, AdjWs* out) {
  AdjWs w;
  c.at = mc_status_layout(batch, c.base, &w.bins);
  w.sort = c.sort(6 * F);
  w.flag = (int32_t*)c.take(6 * F * sizeof(int32_t));
  w.scan = (int32_t*)c.take((6 * F + 1) * sizeof(int32_t));
  w.scan_ws = c.take(ofx_scan_ws_bytes(6 * F));
  w.run = (int32_t*)c.take((6 * F + 1) * sizeof(int32_t));
  if (out) *out = w;
  return c.at;
}

// first position of sk [n] (ascending) whose key is not below `key`
__device__ __forceinline__ int64_t sm_lower(const int64_t* __restrict__ sk, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (sk[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the indices of face t if it takes part: its shape is not refused, they lie inside the shape and differ
__device__ __forceinline__ bool sm_part(const McMesh& m, const int32_t* __restrict__ status, int64_t t, int& b,
                                        int32_t (&id)[3]) {
  b = ms_shape_of(m.tri_off, m.batch, t);
  return !status[b] && mc_face(m, t, b, id) && !mc_degenerate(id);
}

// PAIRS: pair h = 6 t + 2 k + d goes from corner k of face t to the corner d + 1 after it.  Else: corner c = 3 t + k.
template <bool PAIRS>
__global__ __launch_bounds__(MC_T) void adj_key_kernel(McMesh m, McSort s, const int32_t* __restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t t = (int64_t)blockIdx.x * MC_T + threadIdx.x; t < m.F; t += stride) {
    int b;
    int32_t id[3];
    const bool part = sm_part(m, status, t, b, id);
    const int64_t v0 = m.vert_off[b];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (PAIRS) {
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const int64_t h = t * 6 + k * 2 + d;
          s.key[h] = part ? ((v0 + id[k]) << 31) | (v0 + id[(k + 1 + d) % 3]) : MC_NONE;
          s.idx[h] = (int32_t)h;
        }
      } else {
        s.key[t * 3 + k] = part ? v0 + id[k] : MC_NONE;
        s.idx[t * 3 + k] = (int32_t)(t * 3 + k);
      }
    }
  }
}

__global__ __launch_bounds__(MC_T) void adj_flag_kernel(int64_t n6, AdjWs w) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  const int64_t* __restrict__ sk = w.sort.skey;
  for (int64_t p = (int64_t)blockIdx.x * MC_T + threadIdx.x; p < n6; p += stride)
    w.flag[p] = sk[p] != MC_NONE && (p == 0 || sk[p] != sk[p - 1]) ? 1 : 0;
}

// Every head writes its neighbour into its slot (LOCAL: as an index of its shape) and where its run begins; the run
// after the last begins where the pairs that take part end.
template <bool LOCAL>
__global__ __launch_bounds__(MC_T) void adj_fill_kernel(McMesh m, int64_t n6, AdjWs w, int32_t* __restrict__ nbr) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  const int64_t* __restrict__ sk = w.sort.skey;
  for (int64_t p = (int64_t)blockIdx.x * MC_T + threadIdx.x; p < n6; p += stride) {
    if (p == 0) w.run[w.scan[n6]] = (int32_t)sm_lower(sk, n6, MC_NONE);
    if (!w.flag[p]) continue;
    const int64_t u = sk[p] >> 31, v = sk[p] & 0x7fffffff;
    const int32_t r = w.scan[p];
    nbr[r] = (int32_t)(LOCAL ? v - m.vert_off[ms_shape_of(m.vert_off, m.batch, u)] : v);
    w.run[r] = (int32_t)p;
  }
}

// row_off [V + 1], and the flags of every vertex of a shape that is not refused, from the run lengths of its row
__global__ __launch_bounds__(MC_T) void adj_row_kernel(McMesh m, int64_t n6, AdjWs w,
                                                       const int32_t* __restrict__ status,
                                                       int64_t* __restrict__ row_off, int32_t* __restrict__ vflags) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  const int64_t* __restrict__ sk = w.sort.skey;
  for (int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x; i <= m.V; i += stride) {
    const int32_t r0 = w.scan[sm_lower(sk, n6, i << 31)];
    row_off[i] = r0;
    if (i == m.V || status[ms_shape_of(m.vert_off, m.batch, i)]) continue;
    const int32_t r1 = w.scan[sm_lower(sk, n6, (i + 1) << 31)];
    int32_t f = r1 > r0 ? 1 : 0;
    for (int32_t r = r0; r < r1; ++r) {
      const int32_t n = w.run[r + 1] - w.run[r];
      f |= n == 1 ? 2 : (n >= 3 ? 4 : 0);
    }
    vflags[i] = f;
  }
}

// corner_off [V + 1] and the corners, as 3 face + k of their shape, in the sorted order
__global__ __launch_bounds__(MC_T) void adj_corner_kernel(McMesh m, McSort s, int64_t* __restrict__ corner_off,
                                                          int32_t* __restrict__ corner) {
  const int64_t n3 = m.F * 3;
  const int64_t n = n3 > m.V + 1 ? n3 : m.V + 1;
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t p = (int64_t)blockIdx.x * MC_T + threadIdx.x; p < n; p += stride) {
    if (p <= m.V) corner_off[p] = sm_lower(s.skey, n3, p);
    if (p < n3 && s.skey[p] != MC_NONE) {
      const int64_t c = s.sidx[p];
      corner[p] = (int32_t)(c - 3 * m.tri_off[ms_shape_of(m.tri_off, m.batch, c / 3)]);
    }
  }
}

// status -> pairs -> sort -> heads -> scan -> slots -> rows
template <bool LOCAL>
int adj_build(const McMesh& m, const AdjWs& w, int64_t* row_off, int32_t* nbr, int32_t* vflags, int32_t* status,
              void* stream) {
  hipStream_t st = ofx_stream(stream);
  const int64_t n6 = 6 * m.F;
  int rc;
  adj_key_kernel<true><<<ofx_grid(m.F, MC_T), MC_T, 0, st>>>(m, w.sort, status);
  OFX_LAUNCH_CHECK();
  if ((rc = mc_sort(w.sort, n6, stream))) return rc;
  adj_flag_kernel<<<ofx_grid(n6, MC_T), MC_T, 0, st>>>(n6, w);
  OFX_LAUNCH_CHECK();
  if ((rc = ofx_scan_i32(w.flag, w.scan, n6, w.scan_ws, stream))) return rc;
  adj_fill_kernel<LOCAL><<<ofx_grid(n6, MC_T), MC_T, 0, st>>>(m, n6, w, nbr);
  OFX_LAUNCH_CHECK();
  adj_row_kernel<<<ofx_grid(m.V + 1, MC_T), MC_T, 0, st>>>(m, n6, w, status, row_off, vflags);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

int adj_corners(const McMesh& m, const AdjWs& w, int64_t* corner_off, int32_t* corner, const int32_t* status,
                void* stream) {
  hipStream_t st = ofx_stream(stream);
  adj_key_kernel<false><<<ofx_grid(m.F, MC_T), MC_T, 0, st>>>(m, w.sort, status);
  OFX_LAUNCH_CHECK();
  const int rc = mc_sort(w.sort, 3 * m.F, stream);
  if (rc) return rc;
  const int64_t n = 3 * m.F > m.V + 1 ? 3 * m.F : m.V + 1;
  adj_corner_kernel<<<ofx_grid(n, MC_T), MC_T, 0, st>>>(m, w.sort, corner_off, corner);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

// ---- vertex normals -------------------------------------------------------------------------------------------------
struct NrmWs {
  AdjWs adj;
  int64_t* corner_off;            // [V + 1]
  int32_t* corner;                // [3 F]
};
size_t nrm_layout(int batch, int64_t V, int64_t F, char* base, NrmWs* out) {
  Carver c{base};
  NrmWs w;
  adj_layout(batch, F, c, &w.adj);
  w.corner_off = (int64_t*)c.take((V + 1) * sizeof(int64_t));
  w.corner = (int32_t*)c.take(3 * F * sizeof(int32_t));
  if (out) *out = w;
  return c.at;
}

__device__ __forceinline__ void sm_point(const float* __restrict__ verts, int64_t i, double (&p)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = (double)verts[i * 3 + a];
}

template <int MODE>
__global__ __launch_bounds__(MC_T) void nrm_kernel(McMesh m, NrmWs w, const int32_t* __restrict__ status,
                                                   float* __restrict__ normals) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x; i < m.V; i += stride) {
    const int b = ms_shape_of(m.vert_off, m.batch, i);
    if (status[b]) continue;
    const int64_t t0 = m.tri_off[b], v0 = m.vert_off[b];
    double sum[3] = {0.0, 0.0, 0.0};
    for (int64_t p = w.corner_off[i]; p < w.corner_off[i + 1]; ++p) {
      const int32_t c = w.corner[p];
      const int64_t t = t0 + c / 3;
      const int k = c % 3;
      float q[9];
      double n[3];
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int a = 0; a < 3; ++a) q[j * 3 + a] = m.verts[(v0 + m.faces[t * 3 + j]) * 3 + a];
      mc_normal(q, n);
      if (mc_flat(n)) continue;
      double term[3] = {n[0], n[1], n[2]};
      if (MODE != 0) {
        const double len = sqrt(ms_dot(n, n));
        double scale = 1.0;
        if (MODE == 1) {
          double u[3], v[3], x[3];
          const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            u[a] = (double)q[k1 * 3 + a] - (double)q[k * 3 + a];
            v[a] = (double)q[k2 * 3 + a] - (double)q[k * 3 + a];
          }
          ms_cross(u, v, x);
          scale = atan2(sqrt(ms_dot(x, x)), ms_dot(u, v));
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) term[a] = (n[a] / len) * scale;
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) sum[a] += term[a];
    }
    const double len = sqrt(ms_dot(sum, sum));
#pragma unroll
    for (int a = 0; a < 3; ++a) normals[i * 3 + a] = len > 0.0 ? (float)(sum[a] / len) : 0.f;
  }
}

// ---- smoothing ------------------------------------------------------------------------------------------------------
struct SmoothWs {
  AdjWs adj;
  int64_t* row_off;               // [V + 1]
  int32_t* nbr;                   // [6 F] neighbours as indices of the whole call
  int32_t *vflags, *rule;         // [V]
  double* wgt;                    // [6 F] cotangent weights (weights == 1 only)
  double* state[2];               // [V, 3]
};
size_t smooth_layout(int batch, int64_t V, int64_t F, int weights, char* base, SmoothWs* out) {
  Carver c{base};
  SmoothWs w;
  adj_layout(batch, F, c, &w.adj);
  w.row_off = (int64_t*)c.take((V + 1) * sizeof(int64_t));
  w.nbr = (int32_t*)c.take(6 * F * sizeof(int32_t));
  w.vflags = (int32_t*)c.take(V * sizeof(int32_t));
  w.rule = (int32_t*)c.take(V * sizeof(int32_t));
  w.wgt = weights ? (double*)c.take(6 * F * sizeof(double)) : nullptr;
  w.state[0] = (double*)c.take(V * 3 * sizeof(double));
  w.state[1] = (double*)c.take(V * 3 * sizeof(double));
  if (out) *out = w;
  return c.at;
}

// the rule of every vertex, and the input widened into the first buffer
__global__ __launch_bounds__(MC_T) void sm_rule_kernel(McMesh m, SmoothWs w, const int32_t* __restrict__ status,
                                                       int boundary) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x; i < m.V; i += stride) {
#pragma unroll
    for (int a = 0; a < 3; ++a) w.state[0][i * 3 + a] = (double)m.verts[i * 3 + a];
    int32_t rule = SM_REFUSED;
    if (!status[ms_shape_of(m.vert_off, m.batch, i)]) {
      const int32_t f = w.vflags[i];
      rule = !(f & 1) ? SM_PINNED : (!(f & 2) || boundary == 2 ? SM_MOVES : (boundary == 1 ? SM_SLIDES : SM_PINNED));
    }
    w.rule[i] = rule;
  }
}

// Cotangent weight of every neighbour slot: over the faces of its run, the cotangent at the corner opposite the edge.
__global__ __launch_bounds__(MC_T) void sm_cot_kernel(McMesh m, int64_t n6, SmoothWs w) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  const int64_t slots = w.adj.scan[n6];
  for (int64_t r = (int64_t)blockIdx.x * MC_T + threadIdx.x; r < slots; r += stride) {
    double sum = 0.0;
    for (int32_t p = w.adj.run[r]; p < w.adj.run[r + 1]; ++p) {
      const int64_t h = w.adj.sort.sidx[p], t = h / 6;
      const int k = (int)(h % 6) >> 1, d = (int)(h & 1);
      const int64_t v0 = m.vert_off[ms_shape_of(m.tri_off, m.batch, t)];
      double pu[3], pv[3], po[3], u[3], v[3], x[3];
      sm_point(m.verts, v0 + m.faces[t * 3 + k], pu);
      sm_point(m.verts, v0 + m.faces[t * 3 + (k + 1 + d) % 3], pv);
      sm_point(m.verts, v0 + m.faces[t * 3 + (k + 2 - d) % 3], po);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        u[a] = pu[a] - po[a];
        v[a] = pv[a] - po[a];
      }
      ms_cross(u, v, x);
      const double len = sqrt(ms_dot(x, x));
      sum += len > 0.0 ? ms_dot(u, v) / len : 0.0;
    }
    const double half = 0.5 * sum;
    w.wgt[r] = half > 0.0 ? half : 0.0;
  }
}

// One half-step: dst_i = src_i + s (sum_j w_ij (src_j - src_i)) / sum_j w_ij over row i, ascending.
template <bool COT>
__global__ __launch_bounds__(MC_T) void sm_step_kernel(int64_t V, SmoothWs w, const double* __restrict__ src,
                                                       double* __restrict__ dst, double s) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  const int32_t* __restrict__ nbr = w.nbr;
  const int32_t* __restrict__ run = w.adj.run;
  const double* __restrict__ wgt = w.wgt;
  for (int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x; i < V; i += stride) {
    const int32_t rule = w.rule[i];
    double p[3] = {src[i * 3], src[i * 3 + 1], src[i * 3 + 2]};
    if (rule > 0) {
      double acc[3] = {0.0, 0.0, 0.0}, wsum = 0.0;
      const int64_t r1 = w.row_off[i + 1];
      for (int64_t r = w.row_off[i]; r < r1; ++r) {
        const int64_t j = nbr[r];
        const double wij = rule == SM_SLIDES ? (run[r + 1] - run[r] == 1 ? 1.0 : 0.0) : (COT ? wgt[r] : 1.0);
#pragma unroll
        for (int a = 0; a < 3; ++a) acc[a] += wij * (src[j * 3 + a] - p[a]);
        wsum += wij;
      }
      if (wsum > 0.0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = p[a] + s * (acc[a] / wsum);
      }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) dst[i * 3 + a] = p[a];
  }
}

// round once; a pinned vertex keeps the bits it came with
__global__ __launch_bounds__(MC_T) void sm_out_kernel(McMesh m, SmoothWs w, const double* __restrict__ src,
                                                      float* __restrict__ out, double* __restrict__ out64) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x; i < m.V; i += stride) {
    const int32_t rule = w.rule[i];
    if (rule == SM_REFUSED) continue;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double x = src[i * 3 + a];
      if (rule == SM_PINNED) {
        reinterpret_cast<uint32_t*>(out)[i * 3 + a] = reinterpret_cast<const uint32_t*>(m.verts)[i * 3 + a];
      } else {
        out[i * 3 + a] = (float)x;
      }
      if (out64) out64[i * 3 + a] = x;
    }
  }
}

}  // namespace

extern "C" size_t ofx_mesh_adjacency_ws_bytes(int batch, int64_t total_verts, int64_t total_faces) {
  if (!sm_args_ok(batch, total_verts, total_faces)) return 0;
  Carver c{nullptr};
  return adj_layout(batch, total_faces, c, nullptr);
}

extern "C" int ofx_mesh_adjacency(const float* verts, const int32_t* faces, const int64_t* vert_off,
                                  const int64_t* tri_off, int batch, int64_t total_verts, int64_t total_faces,
                                  int64_t* row_off, int32_t* nbr, int32_t* vflags, int64_t* corner_off,
                                  int32_t* corner, void* ws, int32_t* status, void* stream) {
  if (!verts || !faces || !vert_off || !tri_off || !row_off || !nbr || !vflags || !corner_off != !corner || !ws ||
      !status || !sm_args_ok(batch, total_verts, total_faces))
    return OFX_EINVAL;
  const McMesh m{verts, faces, vert_off, tri_off, batch, total_verts, total_faces};
  Carver c{(char*)ws};
  AdjWs w;
  adj_layout(batch, total_faces, c, &w);
  int rc = mc_status(m, w.bins, status, stream);
  if (rc) return rc;
  if (corner && (rc = adj_corners(m, w, corner_off, corner, status, stream))) return rc;
  return adj_build<true>(m, w, row_off, nbr, vflags, status, stream);
}

extern "C" size_t ofx_mesh_vertex_normals_ws_bytes(int batch, int64_t total_verts, int64_t total_faces) {
  if (!sm_args_ok(batch, total_verts, total_faces)) return 0;
  return nrm_layout(batch, total_verts, total_faces, nullptr, nullptr);
}

extern "C" int ofx_mesh_vertex_normals(const float* verts, const int32_t* faces, const int64_t* vert_off,
                                       const int64_t* tri_off, int batch, int64_t total_verts, int64_t total_faces,
                                       int mode, float* normals, void* ws, int32_t* status, void* stream) {
  if (!verts || !faces || !vert_off || !tri_off || !normals || !ws || !status || mode < 0 || mode > 2 ||
      !sm_args_ok(batch, total_verts, total_faces))
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  const McMesh m{verts, faces, vert_off, tri_off, batch, total_verts, total_faces};
  NrmWs w;
  nrm_layout(batch, total_verts, total_faces, (char*)ws, &w);
  int rc = mc_status(m, w.adj.bins, status, stream);
  if (rc) return rc;
  if ((rc = adj_corners(m, w.adj, w.corner_off, w.corner, status, stream))) return rc;
  const int grid = ofx_grid(total_verts, MC_T);
  if (mode == 0) nrm_kernel<0><<<grid, MC_T, 0, st>>>(m, w, status, normals);
  else if (mode == 1) nrm_kernel<1><<<grid, MC_T, 0, st>>>(m, w, status, normals);
  else nrm_kernel<2><<<grid, MC_T, 0, st>>>(m, w, status, normals);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" size_t ofx_mesh_smooth_ws_bytes(int batch, int64_t total_verts, int64_t total_faces, int weights) {
  if (!sm_args_ok(batch, total_verts, total_faces) || weights < 0 || weights > 1) return 0;
  return smooth_layout(batch, total_verts, total_faces, weights, nullptr, nullptr);
}

extern "C" int ofx_mesh_smooth(const float* verts, const int32_t* faces, const int64_t* vert_off,
                               const int64_t* tri_off, int batch, int64_t total_verts, int64_t total_faces, int weights,
                               int boundary, double lambda, double mu, int iters, float* out, double* out64, void* ws,
                               int32_t* status, void* stream) {
  if (!verts || !faces || !vert_off || !tri_off || !out || !ws || !status || weights < 0 || weights > 1 ||
      boundary < 0 || boundary > 2 || !std::isfinite(lambda) || !std::isfinite(mu) || iters < 0 ||
      iters > SM_MAX_ITERS || !sm_args_ok(batch, total_verts, total_faces))
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  const McMesh m{verts, faces, vert_off, tri_off, batch, total_verts, total_faces};
  SmoothWs w;
  smooth_layout(batch, total_verts, total_faces, weights, (char*)ws, &w);
  int rc = mc_status(m, w.adj.bins, status, stream);
  if (rc) return rc;
  if ((rc = adj_build<false>(m, w.adj, w.row_off, w.nbr, w.vflags, status, stream))) return rc;
  const int grid = ofx_grid(total_verts, MC_T);
  sm_rule_kernel<<<grid, MC_T, 0, st>>>(m, w, status, boundary);
  OFX_LAUNCH_CHECK();
  if (weights) {
    sm_cot_kernel<<<ofx_grid(6 * total_faces, MC_T), MC_T, 0, st>>>(m, 6 * total_faces, w);
    OFX_LAUNCH_CHECK();
  }
  int cur = 0;
  for (int it = 0; it < iters; ++it)
    for (int half = 0; half < (mu == 0.0 ? 1 : 2); ++half) {
      const double s = half ? mu : lambda;
      if (weights) sm_step_kernel<true><<<grid, MC_T, 0, st>>>(total_verts, w, w.state[cur], w.state[cur ^ 1], s);
      else sm_step_kernel<false><<<grid, MC_T, 0, st>>>(total_verts, w, w.state[cur], w.state[cur ^ 1], s);
      OFX_LAUNCH_CHECK();
      cur ^= 1;
    }
  sm_out_kernel<<<grid, MC_T, 0, st>>>(m, w, w.state[cur], out, out64);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

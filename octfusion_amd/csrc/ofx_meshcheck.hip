// Is a triangle mesh sound?  Weld equal vertices, count what makes a mesh closed, manifold and oriented, and find the
// faces that intersect other faces.  Contract: include/ofx.h; tests/meshcheck_oracle.py restates it in float64 with
// np.unique and all pairs.  DESIGN.md section 4.22 has the reasons and the figures.
//
//   weld      three stable radix sorts (ofx_points_sort) over the z, y and x bits of every vertex, the shape on top of
//             the last: equal vertices end up side by side in rising index.  Head flags, one scan, and every vertex
//             reads the head of its run.  A second scan, over "is its own representative", numbers the survivors.
//   topology  the 3 F half-edges keyed by their two vertices, the direction in the payload, sorted; every half-edge
//             finds its run by two binary searches.  Duplicate faces: two stable sorts over the sorted triple.
//             Components: ofx_mesh_cc_label / _table, called, not copied.  Area and volume: one wave per shape, 64
//             faces at a time in the wave's butterfly, the chunks in turn (the discipline of ofx_mesh_winding).
//   selfx     one lane per binned triangle, one wave per 64 consecutive records of the shared bins (ofx_tribins.h).
//             The wave walks the bins whose exact box meets its own, stages a bin's records through LDS 64 at a time,
//             and every lane puts the staged faces whose box meets its own through the pair rule.  A pair is judged
//             twice, once from either side, by one function of the ordered pair (the lower index first): counts and
//             minima only, so bins and order decide what is skipped and nothing else.
// Integer atomics only count; no floating-point atomics.
#pragma clang fp contract(off)

#include "ofx_meshtopo.h"

namespace {

constexpr int MC_K = OFX_MESH_TOPOLOGY_K;
constexpr int64_t MC_MAX_F = (int64_t(1) << 30) / 3;

enum { C_DEG, C_EDGES, C_BOUNDARY, C_NONMANIFOLD, C_INCONSISTENT, C_DUPLICATE, C_ZERO_AREA, C_UNREF, C_COMPONENTS };

bool mc_args_ok(int batch, int64_t V, int64_t F) {
  return batch >= 1 && batch <= 65535 && V >= 1 && V <= MC_MAX_V && F >= 1 && F <= MC_MAX_F;
}

// ---- weld ---------------------------------------------------------------------------------------------------------
// coordinate a of vertex i as the bits that decide equality: -0 is +0
__device__ __forceinline__ uint32_t wd_bits(const float* __restrict__ verts, int64_t i, int a) {
  const uint32_t u = (uint32_t)__float_as_int(verts[i * 3 + a]);
  return u == 0x80000000u ? 0u : u;
}
__device__ __forceinline__ bool wd_finite(const float* __restrict__ verts, int64_t i) {
  return isfinite(verts[i * 3]) && isfinite(verts[i * 3 + 1]) && isfinite(verts[i * 3 + 2]);
}

// PASS 0: key = z bits of vertex i, in vertex order.  1: y bits, 2: shape << 32 | x bits, in the order of the sort
// before (stable: the earlier keys break the ties of the later ones).
template <int PASS>
__global__ __launch_bounds__(MC_T) void wd_key_kernel(McMesh m, McSort s) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t p = (int64_t)blockIdx.x * MC_T + threadIdx.x; p < m.V; p += stride) {
    const int64_t i = PASS == 0 ? p : (int64_t)s.sidx[p];
    uint64_t key = wd_bits(m.verts, i, 2 - PASS);
    if (PASS == 2) key |= (uint64_t)ms_shape_of(m.vert_off, m.batch, i) << 32;
    s.key[p] = (int64_t)key;
    s.idx[p] = (int32_t)i;
  }
}

// flag[p] = the vertex at sorted position p starts a run: another shape, another coordinate, or not finite
__global__ __launch_bounds__(MC_T) void wd_flag_kernel(McMesh m, McSort s, int32_t* __restrict__ flag) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t p = (int64_t)blockIdx.x * MC_T + threadIdx.x; p < m.V; p += stride) {
    const int64_t i = s.sidx[p];
    bool head = p == 0 || s.skey[p] != s.skey[p - 1] || !wd_finite(m.verts, i);
    if (!head) {
      const int64_t j = s.sidx[p - 1];
      head = wd_bits(m.verts, i, 1) != wd_bits(m.verts, j, 1) || wd_bits(m.verts, i, 2) != wd_bits(m.verts, j, 2);
    }
    flag[p] = head ? 1 : 0;
  }
}

// head[r] = the vertex that starts run r (the lowest index of the run: the sorts are stable)
__global__ __launch_bounds__(MC_T) void wd_head_kernel(McMesh m, McSort s, const int32_t* __restrict__ flag,
                                                       const int32_t* __restrict__ scan, int32_t* __restrict__ head) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t p = (int64_t)blockIdx.x * MC_T + threadIdx.x; p < m.V; p += stride)
    if (flag[p]) head[scan[p]] = s.sidx[p];
}

__global__ __launch_bounds__(MC_T) void wd_rep_kernel(McMesh m, McSort s, const int32_t* __restrict__ flag,
                                                      const int32_t* __restrict__ scan,
                                                      const int32_t* __restrict__ head,
                                                      const int32_t* __restrict__ status, int32_t* __restrict__ rep,
                                                      int64_t* __restrict__ distinct) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  const int64_t n = m.V > m.batch ? m.V : (int64_t)m.batch;
  for (int64_t p = (int64_t)blockIdx.x * MC_T + threadIdx.x; p < n; p += stride) {
    if (p < m.V) {
      const int64_t i = s.sidx[p];
      const int b = ms_shape_of(m.vert_off, m.batch, i);
      if (!status[b]) rep[i] = (int32_t)((int64_t)head[scan[p] + flag[p] - 1] - m.vert_off[b]);
    }
    // a shape's vertices fill the sorted positions of its own range: the runs that start there are its own
    if (p < m.batch && !status[p]) distinct[p] = (int64_t)scan[m.vert_off[p + 1]] - (int64_t)scan[m.vert_off[p]];
  }
}

// flag[i] = vertex i is its own representative (0 for a shape with a status, or a rep outside its shape)
__global__ __launch_bounds__(MC_T) void we_flag_kernel(McMesh m, const int32_t* __restrict__ rep,
                                                       const int32_t* __restrict__ status, int32_t* __restrict__ flag) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x; i < m.V; i += stride) {
    const int b = ms_shape_of(m.vert_off, m.batch, i);
    flag[i] = !status[b] && (int64_t)rep[i] == i - m.vert_off[b] ? 1 : 0;
  }
}

__global__ __launch_bounds__(MC_T) void we_verts_kernel(McMesh m, const int32_t* __restrict__ rep,
                                                        const int32_t* __restrict__ status,
                                                        const int32_t* __restrict__ flag,
                                                        const int32_t* __restrict__ scan, float* __restrict__ out_verts,
                                                        int32_t* __restrict__ index) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x; i < m.V; i += stride) {
    const int b = ms_shape_of(m.vert_off, m.batch, i);
    if (status[b]) continue;
    const int64_t v0 = m.vert_off[b], nv = m.vert_off[b + 1] - v0;
    const int64_t r = rep[i];
    if (r < 0 || r >= nv || !flag[v0 + r]) continue;          // not what ofx_mesh_weld wrote: nothing is read through it
    index[i] = scan[v0 + r] - scan[v0];
    if (flag[i]) {
#pragma unroll
      for (int a = 0; a < 3; ++a) out_verts[(int64_t)scan[i] * 3 + a] = m.verts[i * 3 + a];
    }
  }
}

__global__ __launch_bounds__(MC_T) void we_faces_kernel(McMesh m, const int32_t* __restrict__ status,
                                                        const int32_t* __restrict__ index,
                                                        int32_t* __restrict__ out_faces) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t t = (int64_t)blockIdx.x * MC_T + threadIdx.x; t < m.F; t += stride) {
    const int b = ms_shape_of(m.tri_off, m.batch, t);
    int32_t id[3];
    if (status[b] || !mc_face(m, t, b, id)) continue;
#pragma unroll
    for (int k = 0; k < 3; ++k) out_faces[t * 3 + k] = index[m.vert_off[b] + id[k]];
  }
}

struct WeldWs {
  TbBins bins;
  McSort sort;
  int32_t *flag, *scan, *head;
  void* scan_ws;
};
size_t weld_layout(int batch, int64_t V, char* base, WeldWs* out) {
  Carver c{base};
  WeldWs w;
  c.at = mc_status_layout(batch, base, &w.bins);
  w.sort = c.sort(V);
  w.flag = (int32_t*)c.take(V * sizeof(int32_t));
  w.scan = (int32_t*)c.take((V + 1) * sizeof(int32_t));
  w.head = (int32_t*)c.take(V * sizeof(int32_t));
  w.scan_ws = c.take(ofx_scan_ws_bytes(V));
  if (out) *out = w;
  return c.at;
}

// ---- topology -----------------------------------------------------------------------------------------------------
struct TopoWs {
  TbBins bins;
  McSort sort;                    // 3 F half-edges, then F faces
  int32_t* ref;                   // [V] a face that takes part uses the vertex
  unsigned long long* acc;        // [batch, MC_K]
  int32_t *label, *comp_off, *cc_status;
  void* cc_ws;
};
size_t topo_layout(int batch, int64_t V, int64_t F, char* base, TopoWs* out) {
  Carver c{base};
  TopoWs w;
  c.at = mc_status_layout(batch, base, &w.bins);
  w.sort = c.sort(3 * F);
  w.ref = (int32_t*)c.take(V * sizeof(int32_t));
  w.acc = (unsigned long long*)c.take((size_t)batch * MC_K * sizeof(unsigned long long));
  w.label = (int32_t*)c.take(V * sizeof(int32_t));
  w.comp_off = (int32_t*)c.take(((size_t)batch + 1) * sizeof(int32_t));
  w.cc_status = (int32_t*)c.take(2 * sizeof(int32_t));
  w.cc_ws = c.take(ofx_mesh_cc_ws_bytes(V, F, batch));
  if (out) *out = w;
  return c.at;
}

__global__ __launch_bounds__(MC_T) void tp_init_kernel(McMesh m, TopoWs w) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x; i < m.V; i += stride) {
    w.ref[i] = 0;
    if (i < (int64_t)m.batch * MC_K) w.acc[i] = 0ull;
  }
  // V >= 1 but batch * MC_K may exceed it
  for (int64_t i = m.V + (int64_t)blockIdx.x * MC_T + threadIdx.x; i < (int64_t)m.batch * MC_K; i += stride)
    w.acc[i] = 0ull;
}

// The three half-edges of every face: key = lower vertex << 31 | higher vertex (indices of the whole call, so a key
// names its shape too), payload = half-edge << 1 | (the face walks it from the higher to the lower vertex).
__global__ __launch_bounds__(MC_T) void tp_halfedge_kernel(McMesh m, TopoWs w, const int32_t* __restrict__ status,
                                                           int32_t* __restrict__ edge_faces) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t t = (int64_t)blockIdx.x * MC_T + threadIdx.x; t < m.F; t += stride) {
    const int b = ms_shape_of(m.tri_off, m.batch, t);
    int32_t id[3];
    const bool ok = !status[b] && mc_face(m, t, b, id);
    const bool part = ok && !mc_degenerate(id);
    const int64_t v0 = m.vert_off[b];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int64_t h = t * 3 + k;
      int64_t key = MC_NONE;
      int rev = 0;
      if (part) {
        const int64_t u = v0 + id[k], v = v0 + id[(k + 1) % 3];
        rev = u > v ? 1 : 0;
        key = ((rev ? v : u) << 31) | (rev ? u : v);
        w.ref[u] = 1;
      }
      w.sort.key[h] = key;
      w.sort.idx[h] = (int32_t)((h << 1) | rev);
      if (ok && !part && edge_faces) edge_faces[h] = 0;
    }
    if (ok && !part) atomicAdd(&w.acc[b * MC_K + C_DEG], 1ull);
    if (part) {
      float c[9];
      double n[3];
      if (ms_load(m.verts, m.faces, m.vert_off, t, b, c)) {
        mc_normal(c, n);
        if (mc_flat(n)) atomicAdd(&w.acc[b * MC_K + C_ZERO_AREA], 1ull);
      }
    }
  }
}

// Every sorted half-edge finds its run [lo, hi) of equal keys; the first of a run counts the edge.
__global__ __launch_bounds__(MC_T) void tp_runs_kernel(McMesh m, TopoWs w, int32_t* __restrict__ edge_faces) {
  const int64_t n3 = m.F * 3;
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  const int64_t* __restrict__ sk = w.sort.skey;
  for (int64_t p = (int64_t)blockIdx.x * MC_T + threadIdx.x; p < n3; p += stride) {
    const int64_t key = sk[p];
    if (key == MC_NONE) continue;
    int64_t lo = 0, hi = p;                       // first position with sk >= key
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (sk[mid] < key) lo = mid + 1; else hi = mid;
    }
    const int64_t first = lo;
    lo = p + 1, hi = n3;                          // first position with sk > key
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (sk[mid] <= key) lo = mid + 1; else hi = mid;
    }
    const int64_t n = lo - first;
    const bool bad = n == 2 && ((w.sort.sidx[first] ^ w.sort.sidx[first + 1]) & 1) == 0;
    const int64_t h = (int64_t)(w.sort.sidx[p] >> 1);
    if (edge_faces) edge_faces[h] = (int32_t)(bad ? -n : n);
    if (p == first) {
      const int b = ms_shape_of(m.tri_off, m.batch, h / 3);
      unsigned long long* acc = w.acc + (int64_t)b * MC_K;
      atomicAdd(&acc[C_EDGES], 1ull);
      if (n == 1) atomicAdd(&acc[C_BOUNDARY], 1ull);
      if (n >= 3) atomicAdd(&acc[C_NONMANIFOLD], 1ull);
      if (bad) atomicAdd(&acc[C_INCONSISTENT], 1ull);
    }
  }
}

// the sorted triple of a face in indices of the whole call; false if it takes no part
__device__ __forceinline__ bool tp_triple(const McMesh& m, const int32_t* __restrict__ status, int64_t t,
                                          int64_t (&s)[3]) {
  const int b = ms_shape_of(m.tri_off, m.batch, t);
  int32_t id[3];
  if (status[b] || !mc_face(m, t, b, id) || mc_degenerate(id)) return false;
  const int64_t v0 = m.vert_off[b];
  const int64_t x = v0 + id[0], y = v0 + id[1], z = v0 + id[2];
  s[0] = x < y ? (x < z ? x : z) : (y < z ? y : z);
  s[2] = x > y ? (x > z ? x : z) : (y > z ? y : z);
  s[1] = x + y + z - s[0] - s[2];
  return true;
}

// PASS 0: key = middle << 31 | highest of face t, in face order; 1: key = lowest, in the order of the first sort
template <int PASS>
__global__ __launch_bounds__(MC_T) void tp_facekey_kernel(McMesh m, TopoWs w, const int32_t* __restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t p = (int64_t)blockIdx.x * MC_T + threadIdx.x; p < m.F; p += stride) {
    const int64_t t = PASS == 0 ? p : (int64_t)w.sort.sidx[p];
    int64_t s[3];
    const bool part = tp_triple(m, status, t, s);
    w.sort.key[p] = part ? (PASS == 0 ? (s[1] << 31) | s[2] : s[0]) : MC_NONE;
    w.sort.idx[p] = (int32_t)t;
  }
}

// a face whose predecessor in (triple, face index) order has its triple repeats a lower-indexed face
__global__ __launch_bounds__(MC_T) void tp_dup_kernel(McMesh m, TopoWs w, const int32_t* __restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t p = 1 + (int64_t)blockIdx.x * MC_T + threadIdx.x; p < m.F; p += stride) {
    int64_t s[3], q[3];
    const int64_t t = w.sort.sidx[p];
    if (!tp_triple(m, status, t, s) || !tp_triple(m, status, w.sort.sidx[p - 1], q)) continue;
    if (s[0] == q[0] && s[1] == q[1] && s[2] == q[2])
      atomicAdd(&w.acc[(int64_t)ms_shape_of(m.tri_off, m.batch, t) * MC_K + C_DUPLICATE], 1ull);
  }
}

__global__ __launch_bounds__(MC_T) void tp_unref_kernel(McMesh m, TopoWs w, const int32_t* __restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * MC_T;
  for (int64_t i = (int64_t)blockIdx.x * MC_T + threadIdx.x; i < m.V; i += stride) {
    const int b = ms_shape_of(m.vert_off, m.batch, i);
    if (!status[b] && !w.ref[i]) atomicAdd(&w.acc[(int64_t)b * MC_K + C_UNREF], 1ull);
  }
}

__device__ __forceinline__ double mc_wave_sum(double v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
  return v;
}

// One wave per shape: area and volume in face order, 64 at a time; then the shape's row of counts.
__global__ __launch_bounds__(MS_T) void tp_sums_kernel(McMesh m, TopoWs w, const int32_t* __restrict__ status,
                                                       int64_t* __restrict__ counts, double* __restrict__ sums) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (status[b]) return;
  const int64_t t0 = m.tri_off[b], F = m.tri_off[b + 1] - t0;
  double area = 0.0, vol = 0.0;
  for (int64_t base = 0; base < F; base += MS_T) {
    double ta = 0.0, tv = 0.0;
    const int64_t t = t0 + base + lane;
    int32_t id[3];
    float c[9];
    if (base + lane < F && mc_face(m, t, b, id) && !mc_degenerate(id) &&
        ms_load(m.verts, m.faces, m.vert_off, t, b, c)) {
      double n[3], x[3];
      mc_normal(c, n);
      ta = 0.5 * sqrt(ms_dot(n, n));
      const double A[3] = {(double)c[0], (double)c[1], (double)c[2]};
      const double B[3] = {(double)c[3], (double)c[4], (double)c[5]};
      const double C[3] = {(double)c[6], (double)c[7], (double)c[8]};
      ms_cross(B, C, x);
      tv = ms_dot(A, x) / 6.0;
    }
    area += mc_wave_sum(ta);
    vol += mc_wave_sum(tv);
  }
  if (lane == 0) {
    sums[b * 2] = area;
    sums[b * 2 + 1] = vol;
  }
  if (lane < MC_K) {
    int64_t v = (int64_t)w.acc[(int64_t)b * MC_K + lane];
    // the component passes write nothing when they refuse the call or give up: -1 says so
    if (lane == C_COMPONENTS)
      v = w.cc_status[0] || w.cc_status[1] ? -1 : (int64_t)w.comp_off[b + 1] - (int64_t)w.comp_off[b];
    counts[(int64_t)b * MC_K + lane] = v;
  }
}

// ---- self-intersections: the pair rule -----------------------------------------------------------------------------
// A triangle is a column of LDS: coordinate a of corner k at T[(3 k + a) * MS_T].
__device__ __forceinline__ void sx_corner(const double* T, int k, double (&p)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = T[(3 * k + a) * MS_T];
}
__device__ __forceinline__ void sx_sub(const double (&u)[3], const double (&v)[3], double (&r)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) r[a] = u[a] - v[a];
}
__device__ __forceinline__ int sx_sign(double x) { return x > 0.0 ? 1 : (x < 0.0 ? -1 : 0); }
__device__ __forceinline__ bool sx_one_side(int a, int b, int c) {
  return (a >= 0 && b >= 0 && c >= 0) || (a <= 0 && b <= 0 && c <= 0);
}
// the axes kept when projecting along the dominant axis of n (ties to the lowest index): k + 1 and k + 2
__device__ __forceinline__ void sx_axes(const double (&n)[3], int& u, int& v) {
  int k = 0;
  if (fabs(n[1]) > fabs(n[0])) k = 1;
  if (fabs(n[2]) > fabs(n[k])) k = 2;
  u = k == 2 ? 0 : k + 1;
  v = k == 0 ? 2 : k - 1;
}
struct P2 {
  double x, y;
};
__device__ __forceinline__ P2 sx_drop(const double (&p)[3], int u, int v) {
  return P2{u == 0 ? p[0] : (u == 1 ? p[1] : p[2]), v == 0 ? p[0] : (v == 1 ? p[1] : p[2])};
}
// orientation of p, q, r: the sign of (q - p) x (r - p) on rounded differences
__device__ __forceinline__ int sx_o2(P2 p, P2 q, P2 r) {
  return sx_sign(ms_det2(q.x - p.x, r.y - p.y, q.y - p.y, r.x - p.x));
}
__device__ __forceinline__ bool sx_inside(P2 a, P2 b, P2 c, P2 x) {
  return sx_one_side(sx_o2(a, b, x), sx_o2(b, c, x), sx_o2(c, a, x));
}
__device__ __forceinline__ bool sx_seg_cross(P2 p, P2 q, P2 r, P2 s) {
  const int d1 = sx_o2(p, q, r), d2 = sx_o2(p, q, s), d3 = sx_o2(r, s, p), d4 = sx_o2(r, s, q);
  if (d1 == 0 && d2 == 0 && d3 == 0 && d4 == 0) {
    const bool ax = fabs(q.x - p.x) >= fabs(q.y - p.y);
    const double P = ax ? p.x : p.y, Q = ax ? q.x : q.y, R = ax ? r.x : r.y, S = ax ? s.x : s.y;
    return fmax(fmin(P, Q), fmin(R, S)) <= fmin(fmax(P, Q), fmax(R, S));
  }
  return d1 * d2 <= 0 && d3 * d4 <= 0;
}

// the edge from corner kp to corner kq of E meets the closed triangle T
__device__ __noinline__ bool sx_edge_meets(const double* E, int kp, int kq, const double* T) {
  double p[3], q[3], a[3], b[3], c[3], e1[3], e2[3], n[3], d[3];
  sx_corner(E, kp, p);
  sx_corner(E, kq, q);
  sx_corner(T, 0, a);
  sx_corner(T, 1, b);
  sx_corner(T, 2, c);
  sx_sub(b, a, e1);
  sx_sub(c, a, e2);
  ms_cross(e1, e2, n);
  sx_sub(p, a, d);
  const int sp = sx_sign(ms_dot(n, d));
  sx_sub(q, a, d);
  const int sq = sx_sign(ms_dot(n, d));
  if (sp == sq && sp != 0) return false;
  if (sp == 0 && sq == 0) {
    int u, v;
    sx_axes(n, u, v);
    const P2 P = sx_drop(p, u, v), Q = sx_drop(q, u, v), A = sx_drop(a, u, v), B = sx_drop(b, u, v),
             C = sx_drop(c, u, v);
    return sx_inside(A, B, C, P) || sx_inside(A, B, C, Q) || sx_seg_cross(P, Q, A, B) || sx_seg_cross(P, Q, B, C) ||
           sx_seg_cross(P, Q, C, A);
  }
  double A[3], B[3], C[3], x[3];
  sx_sub(q, p, d);
  sx_sub(a, p, A);
  sx_sub(b, p, B);
  sx_sub(c, p, C);
  ms_cross(A, B, x);
  const int o1 = sx_sign(ms_dot(d, x));
  ms_cross(B, C, x);
  const int o2 = sx_sign(ms_dot(d, x));
  ms_cross(C, A, x);
  const int o3 = sx_sign(ms_dot(d, x));
  return sx_one_side(o1, o2, o3);
}

// k = 2: I's corner `apex` is the one J does not share, J's corner `other` the one I does not
__device__ __noinline__ bool sx_fold(const double* I, int apex, const double* J, int other) {
  double a0[3], a1[3], a2[3], e1[3], e2[3], n[3], b[3], d[3], a[3], u3[3], v3[3];
  sx_corner(I, 0, a0);
  sx_corner(I, 1, a1);
  sx_corner(I, 2, a2);
  sx_sub(a1, a0, e1);
  sx_sub(a2, a0, e2);
  ms_cross(e1, e2, n);
  sx_corner(J, other, b);
  sx_sub(b, a0, d);
  if (ms_dot(n, d) != 0.0) return false;
  sx_corner(I, apex, a);
  sx_corner(I, (apex + 1) % 3, u3);
  sx_corner(I, (apex + 2) % 3, v3);
  int u, v;
  sx_axes(n, u, v);
  const P2 U = sx_drop(u3, u, v), W = sx_drop(v3, u, v);
  const int sa = sx_o2(U, W, sx_drop(a, u, v)), sb = sx_o2(U, W, sx_drop(b, u, v));
  return sa != 0 && sa == sb;
}

// The rule of the ordered pair: I the lower-indexed face with indices fi, J the higher with fj.
__device__ __forceinline__ bool sx_pair(const double* I, const int32_t (&fi)[3], const double* J,
                                        const int32_t (&fj)[3]) {
  int k = 0, si = 0, sj = 0;                      // bit m of si: corner m of I is shared
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      if (fi[a] == fj[b]) {
        ++k;
        si |= 1 << a;
        sj |= 1 << b;
      }
  if (k >= 3) return false;
  if (k == 2) return sx_fold(I, si == 3 ? 2 : (si == 5 ? 1 : 0), J, sj == 3 ? 2 : (sj == 5 ? 1 : 0));
  if (k == 1) {
    const int pi = si == 1 ? 0 : (si == 2 ? 1 : 2), pj = sj == 1 ? 0 : (sj == 2 ? 1 : 2);
    return sx_edge_meets(I, (pi + 1) % 3, (pi + 2) % 3, J) || sx_edge_meets(J, (pj + 1) % 3, (pj + 2) % 3, I);
  }
  bool hit = false;
#pragma unroll 1
  for (int e = 0; e < 6 && !hit; ++e) {
    const int kp = e % 3, kq = (e + 1) % 3;
    hit = e < 3 ? sx_edge_meets(I, kp, kq, J) : sx_edge_meets(J, kp, kq, I);
  }
  return hit;
}

template <bool COUNT>
__global__ __launch_bounds__(MS_T) void sx_kernel(TbMesh m, TbBins w, const int32_t* __restrict__ status,
                                                  int32_t* __restrict__ partners, int32_t* __restrict__ first,
                                                  unsigned long long* counters) {
  __shared__ double own[9 * MS_T], rec[9 * MS_T];
  __shared__ float sbox[6 * MS_T];
  __shared__ int32_t sidx[4 * MS_T];             // three vertex indices and the face
  const int b = blockIdx.y;
  if (status[b]) return;
  const int64_t bin0 = (int64_t)b * m.GS;
  const int64_t r0 = w.off[bin0], nrec = (int64_t)w.off[bin0 + m.GS] - r0;      // the shape's records
  if ((int64_t)blockIdx.x * MS_T >= nrec) return;
  const int lane = threadIdx.x;
  const int64_t t0 = m.tri_off[b], F = m.tri_off[b + 1] - t0;
  const int G = tb_G(m, b), G3 = G * G * G;

  // the lane's own triangle
  const int64_t s = (int64_t)blockIdx.x * MS_T + lane;
  int32_t me = -1, fme[3] = {-1, -2, -3};
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  bool live = false;
  if (s < nrec) {
    float c[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) c[k] = w.tri[(r0 + s) * TB_W + k];
    me = __float_as_int(w.tri[(r0 + s) * TB_W + 9]);
    if (me >= 0 && (int64_t)me < F) {
#pragma unroll
      for (int k = 0; k < 3; ++k) fme[k] = m.faces[(t0 + me) * 3 + k];
      double n[3];
      mc_normal(c, n);
      live = !mc_flat(n) && !mc_degenerate(fme);
#pragma unroll
      for (int k = 0; k < 9; ++k) own[k * MS_T + lane] = (double)c[k];
      if (live) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          lo[a] = fminf(fminf(c[a], c[3 + a]), c[6 + a]);
          hi[a] = fmaxf(fmaxf(c[a], c[3 + a]), c[6 + a]);
        }
      }
    } else {
      me = -1;
    }
  }
  float wlo[3], whi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    wlo[a] = ms_wave_min(lo[a]);
    whi[a] = ms_wave_max(hi[a]);
  }
  int32_t count = 0, lowest = INT32_MAX;
  uint32_t visited = 0u, staged = 0u, judged = 0u;
  if (__ballot(live) != 0ull) {
    for (int g0 = 0; g0 < G3; g0 += MS_T) {
      const int g = g0 + lane;
      bool cand = false;
      if (g < G3 && w.off[bin0 + g + 1] - w.off[bin0 + g] > 0) {
        float blo[3], bhi[3];
        ms_bin_box(w.box, bin0 + g, blo, bhi);
        cand = blo[0] <= whi[0] && bhi[0] >= wlo[0] && blo[1] <= whi[1] && bhi[1] >= wlo[1] && blo[2] <= whi[2] &&
               bhi[2] >= wlo[2];
      }
      uint64_t bmask = __ballot(cand);
      while (bmask) {
        const int jb = __ffsll((unsigned long long)bmask) - 1;
        bmask &= bmask - 1;
        const int64_t start = w.off[bin0 + g0 + jb];
        const int n = w.off[bin0 + g0 + jb + 1] - (int32_t)start;
        if (COUNT) {
          visited += 1u;
          staged += (uint32_t)n;
        }
        for (int base = 0; base < n; base += MS_T) {
          bool keep = base + lane < n;
          if (keep) {
            float c[9];
            const int64_t r = start + base + lane;
#pragma unroll
            for (int k = 0; k < 9; ++k) c[k] = w.tri[r * TB_W + k];
            const int32_t id = __float_as_int(w.tri[r * TB_W + 9]);
            float tlo[3], thi[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              tlo[a] = fminf(fminf(c[a], c[3 + a]), c[6 + a]);
              thi[a] = fmaxf(fmaxf(c[a], c[3 + a]), c[6 + a]);
            }
            keep = id >= 0 && (int64_t)id < F && tlo[0] <= whi[0] && thi[0] >= wlo[0] && tlo[1] <= whi[1] &&
                   thi[1] >= wlo[1] && tlo[2] <= whi[2] && thi[2] >= wlo[2];
            if (keep) {
              int32_t f[3];
#pragma unroll
              for (int k = 0; k < 3; ++k) f[k] = m.faces[(t0 + id) * 3 + k];
              double nn[3];
              mc_normal(c, nn);
              keep = !mc_flat(nn) && !mc_degenerate(f);
              if (keep) {
#pragma unroll
                for (int k = 0; k < 9; ++k) rec[k * MS_T + lane] = (double)c[k];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                  sbox[a * MS_T + lane] = tlo[a];
                  sbox[(3 + a) * MS_T + lane] = thi[a];
                  sidx[a * MS_T + lane] = f[a];
                }
                sidx[3 * MS_T + lane] = id;
              }
            }
          }
          __syncthreads();
          uint64_t mask = __ballot(keep);
          while (mask) {
            const int j = __ffsll((unsigned long long)mask) - 1;
            mask &= mask - 1;
            const int32_t other = sidx[3 * MS_T + j];
            if (!live || other == me) continue;
            if (!(sbox[j] <= hi[0] && sbox[3 * MS_T + j] >= lo[0] && sbox[MS_T + j] <= hi[1] &&
                  sbox[4 * MS_T + j] >= lo[1] && sbox[2 * MS_T + j] <= hi[2] && sbox[5 * MS_T + j] >= lo[2]))
              continue;
            const int32_t fo[3] = {sidx[j], sidx[MS_T + j], sidx[2 * MS_T + j]};
            if (COUNT) judged += 1u;
            const bool hit = me < other ? sx_pair(own + lane, fme, rec + j, fo) : sx_pair(rec + j, fo, own + lane, fme);
            if (hit) {
              count += 1;
              lowest = other < lowest ? other : lowest;
            }
          }
          __syncthreads();
        }
      }
    }
  }
  if (me >= 0) {
    partners[t0 + me] = count;
    first[t0 + me] = count ? lowest : -1;
  }
  if (COUNT) {
    unsigned long long j = judged;
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) j += __shfl_xor(j, sft);
    if (lane == 0) {
      atomicAdd(&counters[0], (unsigned long long)visited);
      atomicAdd(&counters[1], (unsigned long long)staged);
      atomicAdd(&counters[2], j);
    }
  }
}

// pairs[b] = sum of partners / 2: integers, so the order of the sum is free
__global__ __launch_bounds__(MC_T) void sx_pairs_kernel(TbMesh m, const int32_t* __restrict__ status,
                                                        const int32_t* __restrict__ partners,
                                                        int64_t* __restrict__ pairs) {
  __shared__ long long part[MC_T];
  const int b = blockIdx.x;
  if (status[b]) return;
  const int64_t t0 = m.tri_off[b], F = m.tri_off[b + 1] - t0;
  long long sum = 0;
  for (int64_t t = threadIdx.x; t < F; t += MC_T) sum += partners[t0 + t];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (int s = MC_T / 2; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) pairs[b] = part[0] / 2;
}

unsigned long long* sx_counters = nullptr;      // ofx_mesh_selfx_set_counters

}  // namespace

extern "C" size_t ofx_mesh_weld_ws_bytes(int batch, int64_t total_verts, int64_t total_faces) {
  if (!mc_args_ok(batch, total_verts, total_faces)) return 0;
  return weld_layout(batch, total_verts, nullptr, nullptr);
}

extern "C" int ofx_mesh_weld(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                             int batch, int64_t total_verts, int64_t total_faces, int32_t* rep, int64_t* distinct,
                             void* ws, int32_t* status, void* stream) {
  if (!verts || !faces || !vert_off || !tri_off || !rep || !distinct || !ws || !status ||
      !mc_args_ok(batch, total_verts, total_faces))
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  const McMesh m{verts, faces, vert_off, tri_off, batch, total_verts, total_faces};
  WeldWs w;
  weld_layout(batch, total_verts, (char*)ws, &w);
  int rc = mc_status(m, w.bins, status, stream);
  if (rc) return rc;
  const int grid = ofx_grid(total_verts, MC_T);
  wd_key_kernel<0><<<grid, MC_T, 0, st>>>(m, w.sort);
  OFX_LAUNCH_CHECK();
  if ((rc = mc_sort(w.sort, total_verts, stream))) return rc;
  wd_key_kernel<1><<<grid, MC_T, 0, st>>>(m, w.sort);
  OFX_LAUNCH_CHECK();
  if ((rc = mc_sort(w.sort, total_verts, stream))) return rc;
  wd_key_kernel<2><<<grid, MC_T, 0, st>>>(m, w.sort);
  OFX_LAUNCH_CHECK();
  if ((rc = mc_sort(w.sort, total_verts, stream))) return rc;
  wd_flag_kernel<<<grid, MC_T, 0, st>>>(m, w.sort, w.flag);
  OFX_LAUNCH_CHECK();
  if ((rc = ofx_scan_i32(w.flag, w.scan, total_verts, w.scan_ws, stream))) return rc;
  wd_head_kernel<<<grid, MC_T, 0, st>>>(m, w.sort, w.flag, w.scan, w.head);
  OFX_LAUNCH_CHECK();
  wd_rep_kernel<<<ofx_grid(total_verts > batch ? total_verts : batch, MC_T), MC_T, 0, st>>>(
      m, w.sort, w.flag, w.scan, w.head, status, rep, distinct);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" int ofx_mesh_weld_extract(const float* verts, const int32_t* faces, const int64_t* vert_off,
                                     const int64_t* tri_off, int batch, int64_t total_verts, int64_t total_faces,
                                     const int32_t* rep, const int32_t* status, float* out_verts, int32_t* out_faces,
                                     int32_t* index, void* ws, void* stream) {
  if (!verts || !faces || !vert_off || !tri_off || !rep || !status || !out_verts || !out_faces || !index || !ws ||
      !mc_args_ok(batch, total_verts, total_faces))
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  const McMesh m{verts, faces, vert_off, tri_off, batch, total_verts, total_faces};
  WeldWs w;
  weld_layout(batch, total_verts, (char*)ws, &w);
  const int grid = ofx_grid(total_verts, MC_T);
  we_flag_kernel<<<grid, MC_T, 0, st>>>(m, rep, status, w.flag);
  OFX_LAUNCH_CHECK();
  const int rc = ofx_scan_i32(w.flag, w.scan, total_verts, w.scan_ws, stream);
  if (rc) return rc;
  we_verts_kernel<<<grid, MC_T, 0, st>>>(m, rep, status, w.flag, w.scan, out_verts, index);
  OFX_LAUNCH_CHECK();
  we_faces_kernel<<<ofx_grid(total_faces, MC_T), MC_T, 0, st>>>(m, status, index, out_faces);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" size_t ofx_mesh_topology_ws_bytes(int batch, int64_t total_verts, int64_t total_faces) {
  if (!mc_args_ok(batch, total_verts, total_faces)) return 0;
  return topo_layout(batch, total_verts, total_faces, nullptr, nullptr);
}

extern "C" int ofx_mesh_topology(const float* verts, const int32_t* faces, const int64_t* vert_off,
                                 const int64_t* tri_off, int batch, int64_t total_verts, int64_t total_faces,
                                 int64_t* counts, double* sums, int32_t* edge_faces, void* ws, int32_t* status,
                                 void* stream) {
  if (!verts || !faces || !vert_off || !tri_off || !counts || !sums || !ws || !status ||
      !mc_args_ok(batch, total_verts, total_faces))
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  const McMesh m{verts, faces, vert_off, tri_off, batch, total_verts, total_faces};
  TopoWs w;
  topo_layout(batch, total_verts, total_faces, (char*)ws, &w);
  int rc = mc_status(m, w.bins, status, stream);
  if (rc) return rc;
  const int gv = ofx_grid(total_verts, MC_T), gf = ofx_grid(total_faces, MC_T);
  tp_init_kernel<<<gv, MC_T, 0, st>>>(m, w);
  OFX_LAUNCH_CHECK();
  tp_halfedge_kernel<<<gf, MC_T, 0, st>>>(m, w, status, edge_faces);
  OFX_LAUNCH_CHECK();
  if ((rc = mc_sort(w.sort, 3 * total_faces, stream))) return rc;
  tp_runs_kernel<<<ofx_grid(3 * total_faces, MC_T), MC_T, 0, st>>>(m, w, edge_faces);
  OFX_LAUNCH_CHECK();
  tp_facekey_kernel<0><<<gf, MC_T, 0, st>>>(m, w, status);
  OFX_LAUNCH_CHECK();
  if ((rc = mc_sort(w.sort, total_faces, stream))) return rc;
  tp_facekey_kernel<1><<<gf, MC_T, 0, st>>>(m, w, status);
  OFX_LAUNCH_CHECK();
  if ((rc = mc_sort(w.sort, total_faces, stream))) return rc;
  tp_dup_kernel<<<gf, MC_T, 0, st>>>(m, w, status);
  OFX_LAUNCH_CHECK();
  tp_unref_kernel<<<gv, MC_T, 0, st>>>(m, w, status);
  OFX_LAUNCH_CHECK();
  if ((rc = ofx_mesh_cc_label(faces, vert_off, tri_off, batch, total_verts, total_faces, w.label, w.cc_ws,
                              w.cc_status, stream)))
    return rc;
  if ((rc = ofx_mesh_cc_table(faces, w.label, vert_off, tri_off, batch, total_verts, total_faces, nullptr, w.comp_off,
                              w.cc_ws, w.cc_status, stream)))
    return rc;
  tp_sums_kernel<<<batch, MS_T, 0, st>>>(m, w, status, counts, sums);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" size_t ofx_mesh_selfx_ws_bytes(int batch, int64_t total_verts, int64_t total_faces, int bins) {
  if (!ofx_tribins_args_ok(batch, total_verts, total_faces, 0, bins)) return 0;
  return ofx_tribins_layout(batch, total_faces, 0, bins, nullptr, nullptr, nullptr);
}

extern "C" int ofx_mesh_selfx_set_counters(unsigned long long* words) {
  sx_counters = words;
  return OFX_OK;
}

extern "C" int ofx_mesh_selfx(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                              int batch, int64_t max_faces, int bins, int32_t* partners, int32_t* first, int64_t* pairs,
                              void* ws, int32_t* status, void* stream) {
  if (!verts || !faces || !vert_off || !tri_off || !partners || !first || !pairs || !ws || !status ||
      !ofx_tribins_args_ok(batch, 1, 1, 0, bins) || max_faces < 1 || max_faces > INT32_MAX)
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  TbBins w;
  ofx_tribins_layout(batch, 0, 0, bins, (char*)ws, &w, nullptr);     // the records are last: their size is not needed
  const TbMesh m{verts, faces, vert_off, tri_off, batch, bins, tb_stride(bins)};
  const int rc = ofx_tribins_build(m, w, 1, status, stream);          // 1: fill the bins (there are no queries to order)
  if (rc) return rc;
  const dim3 waves((unsigned)ofx_cdiv(max_faces, MS_T), (unsigned)batch);
  if (sx_counters) sx_kernel<true><<<waves, MS_T, 0, st>>>(m, w, status, partners, first, sx_counters);
  else sx_kernel<false><<<waves, MS_T, 0, st>>>(m, w, status, partners, first, nullptr);
  OFX_LAUNCH_CHECK();
  sx_pairs_kernel<<<batch, MC_T, 0, st>>>(m, status, partners, pairs);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

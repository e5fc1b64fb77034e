// What the kernels that read a mesh as a graph share (ofx_meshcheck.hip, ofx_meshsmooth.hip): the meshes of a call, the
// workspace carver with its (key, index) sort arrays, the status words, a face's three indices and the exact-zero area
// rule.  One copy, so that "takes part" and "flat" mean the same in both files.  Include it after
// `#pragma clang fp contract(off)`: every operation here is rounded on its own.
#pragma once
#include "ofx_tribins.h"

#include <cmath>

#include "ofx_tri.h"

constexpr int MC_T = 256;
constexpr int64_t MC_NONE = INT64_MAX;        // key of a half-edge or a face that takes no part: sorts last
constexpr int64_t MC_MAX_V = int64_t(1) << 30;             // what one ofx_points_sort takes

struct McMesh {
  const float* verts;
  const int32_t* faces;
  const int64_t* vert_off;
  const int64_t* tri_off;
  int batch;
  int64_t V, F;
};

// The (key, index) arrays of a sort of n items and its workspace.
struct McSort {
  int64_t *key, *skey;
  int32_t *idx, *sidx;
  void* ws;
  size_t ws_bytes;
};

struct Carver {
  char* base;
  size_t at = 0;
  char* take(size_t bytes) {
    char* p = base ? base + at : nullptr;
    at += tb_align(bytes);
    return p;
  }
  McSort sort(int64_t n) {
    McSort s;
    s.key = (int64_t*)take(n * sizeof(int64_t));
    s.skey = (int64_t*)take(n * sizeof(int64_t));
    s.idx = (int32_t*)take(n * sizeof(int32_t));
    s.sidx = (int32_t*)take(n * sizeof(int32_t));
    s.ws_bytes = ofx_points_sort_ws_bytes(n);
    s.ws = take(s.ws_bytes);
    return s;
  }
};

static inline int mc_sort(const McSort& s, int64_t n, void* stream) {
  return ofx_points_sort(s.key, s.idx, n, s.skey, s.sidx, s.ws, s.ws_bytes, stream);
}

// The status words of a call: the validation of the shared bin builder, which stops there (no queries).
static inline size_t mc_status_layout(int batch, char* base, TbBins* w) {
  return ofx_tribins_layout(batch, 0, 0, 1, base, w, nullptr);
}
static inline int mc_status(const McMesh& m, const TbBins& w, int32_t* status, void* stream) {
  const TbMesh t{m.verts, m.faces, m.vert_off, m.tri_off, m.batch, 1, tb_stride(1)};
  return ofx_tribins_build(t, w, 0, status, stream);
}

// the three indices of face t of shape b; false if one lies outside the shape
__device__ __forceinline__ bool mc_face(const McMesh& m, int64_t t, int b, int32_t (&id)[3]) {
  const int64_t nv = m.vert_off[b + 1] - m.vert_off[b];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    id[k] = m.faces[t * 3 + k];
    ok = ok && id[k] >= 0 && (int64_t)id[k] < nv;
  }
  return ok;
}
__device__ __forceinline__ bool mc_degenerate(const int32_t (&id)[3]) {
  return id[0] == id[1] || id[1] == id[2] || id[0] == id[2];
}

// (b - a) x (c - a) of the nine coordinates is exactly zero: the rule of ofx_mesh_winding
__device__ __forceinline__ void mc_normal(const float (&c)[9], double (&n)[3]) {
  double e1[3], e2[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    e1[a] = (double)c[3 + a] - (double)c[a];
    e2[a] = (double)c[6 + a] - (double)c[a];
  }
  ms_cross(e1, e2, n);
}
__device__ __forceinline__ bool mc_flat(const double (&n)[3]) { return n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0; }

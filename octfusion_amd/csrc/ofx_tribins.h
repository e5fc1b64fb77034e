// The structure the point queries (ofx_meshquery.hip) and the ray casts (ofx_raycast.hip) search, built once for both
// by ofx_tribins.hip: every valid triangle of a shape goes into ONE bin of a G^3 grid over the shape's OWN bounding box
// (of the vertices its valid faces use) by its clamped centroid; a bin keeps the exact bounding box of its triangles
// and its records, nine coordinates and the face's index, lie together.  One copy, so that "same conditions, same grid
// rule" (include/ofx.h) holds by construction.  Here: what the search kernels need inline, and the three host
// functions of the builder.  DESIGN.md section 4.19.
#pragma once
#include "ofx_common.h"

constexpr int TB_MAX_G = 16;       // at most 16^3 bins per shape
constexpr int TB_PREP_T = 256;
constexpr int TB_W = 10;           // words per binned triangle: nine coordinates and the face's index
constexpr int TB_FACES_PER_G2 = 256;

// The automatic grid: the smallest G in 1 .. 16 with 256 G^2 >= F.  A surface meets about 3 G^2 of the G^3 bins, so
// an occupied bin holds about F / (3 G^2) <= 85 triangles: one or two staging rounds of 64.
__host__ __device__ inline int tb_bins(int64_t F, int bins) {
  if (bins) return bins;
  int g = 1;
  while (g < TB_MAX_G && (int64_t)TB_FACES_PER_G2 * g * g < F) ++g;
  return g;
}
// bins of one shape in the workspace (the stride of the per-bin arrays)
inline int tb_stride(int bins) { return bins ? bins * bins * bins : TB_MAX_G * TB_MAX_G * TB_MAX_G; }

inline size_t tb_align(size_t b) { return (b + 255) & ~(size_t)255; }

// The meshes of one call.  An entry derives its own argument block from it and adds its queries or rays.
struct TbMesh {
  const float* verts;
  const int32_t* faces;
  const int64_t* vert_off;
  const int64_t* tri_off;
  int batch, bins, GS;
};

__device__ __forceinline__ int tb_G(const TbMesh& m, int b) { return tb_bins(m.tri_off[b + 1] - m.tri_off[b], m.bins); }

struct TbBins {
  int32_t* cnt;      // [batch * GS]      triangles per bin
  int32_t* off;      // [batch * GS + 1]  exclusive scan
  int32_t* cursor;   // [batch * GS]      fill cursors
  int32_t* box;      // [batch * GS * 6]  keys of min xyz, max xyz of a bin
  int32_t* sbox;     // [batch * 6]       the same of a shape
  void* scan_ws;
  float* tri;        // [total_faces * 10] records in bin order
};

// Room for an entry to put its Q queries or rays into an order of its own (ofx_points_sort); the builder only lays it
// out.
struct TbOrder {
  int64_t* key;      // [Q] sort keys, [Q] sorted
  int64_t* skey;
  int32_t* idx;      // [Q] index of the query or ray, [Q] sorted
  int32_t* sidx;
  void* sort_ws;
  size_t sort_bytes;
};

// the ranges ofx_mesh_query and ofx_ray_cast accept (include/ofx.h)
bool ofx_tribins_args_ok(int batch, int64_t total_verts, int64_t total_faces, int64_t total_q, int bins);

// Carves the workspace of either entry: the bins' arrays, the order's, and last the records, the only array sized by
// the faces (so total_faces may be 0 where only the pointers are wanted).  Returns the bytes; base, w, o may be NULL.
size_t ofx_tribins_layout(int batch, int64_t total_faces, int64_t total_q, int bins, char* base, TbBins* w, TbOrder* o);

// Zeroes the status words, validates every triangle (status[b] |= 1 for a shape with a bad one) and bounds the shapes;
// then, unless total_q == 0, count -> ofx_scan_i32 -> fill.  OFX_OK or the error of the step that failed.
int ofx_tribins_build(const TbMesh& m, const TbBins& w, int64_t total_q, int32_t* status, void* stream);

// Puts the Q points q [Q, 3] (q_off [batch + 1]: where each shape's begin) into o.sidx so that a wave of 64 consecutive
// slots holds neighbours: key = shape << 32 | non-finite << 30 | 30-bit Morton code of the point clamped into the
// shape's box (of ofx_tribins_build, which must have run), sorted by ofx_points_sort.  A shape's points stay in its own
// range of slots; the order inside it is a performance device only.
int ofx_tribins_order_points(const TbMesh& m, const float* q, const int64_t* q_off, const TbBins& w, const TbOrder& o,
                             int64_t total_q, void* stream);

// Signed distance lattice of a triangle mesh: the reference's offline mesh2sdf.compute call
// (tools/repair_mesh.py:150) on the device.  Contract: include/ofx.h; tests/mesh2sdf_oracle.py restates it in float64
// (brute-force closest point, winding number).  DESIGN.md section 4.11 has the cost model and the exactness argument.
//
//   bins   every valid triangle goes into ONE bin of a G^3 grid over [-1, 1]^3 (G = ceil(S / 8), at most 16) by its
//          clamped centroid; a bin keeps the exact bounding box of its triangles (integer atomicMin / atomicMax on
//          order-preserving keys: order-independent).  count -> ofx_scan_i32 -> fill; the fill copies the nine
//          coordinates into bin order.  The order inside a bin depends on arrival; nothing below depends on it.
//   dist   one wave per brick of 4^3 lattice points, one point per lane.  Pass 1 over the bins: U = min over bins of
//          the LARGEST box-to-box distance (a non-empty bin holds a triangle inside its box, so every point of the
//          brick is within U of the surface); the bin that gives U is searched first.  Pass 2 searches every other
//          bin whose SMALLEST box-to-box distance is within U and within the brick's current worst best.  Inside a
//          bin, 64 triangles at a time: each lane stages one triangle into LDS and culls it by its own box, the
//          survivors are evaluated by all lanes.  Every skip compares a lower bound with an upper bound, with a margin
//          far above the rounding of either, so the minimum is the minimum over ALL triangles of one fixed fp64
//          expression: order-independent, the same alone or in a batch.
//   pair   closest point in fp64: the three edges as clamped segments (a zero-length edge is its end point), and the
//          plane distance where the projection falls inside.  The normal is exact to one rounding (differences and
//          products of fp32 values are exact in fp64), so a zero-area triangle has n == 0 and is its edges: no NaN.
//   sign   one wave per tile of 8 x 8 columns (j, k), one column per lane, same staging.  A triangle counts for a
//          column iff its yz-projection contains the point moved by (eps, eps^2): the three edge functions are
//          evaluated on a canonical ordering of the edge's end points (so the two triangles of an edge get the same
//          bits, negated), a zero is resolved by -sign(dz), then sign(dy).  The crossing's x toggles bit
//          ceil(index of x) of the column's mask in LDS; a prefix-xor along i negates the stored distances.
#include "ofx_common.h"

#include <cmath>

#pragma clang fp contract(off)

#include "ofx_tri.h"          // the bounds, the pair and the crossing: shared with ofx_meshquery.hip

namespace {

constexpr int MS_BRICK = 4;        // one wave (MS_T lanes) per block: a brick of 4^3 points / a tile of 8 x 8 columns
constexpr int MS_TILE = 8;
constexpr int MS_BIN_CELLS = 8;    // lattice cells per bin edge (until the cap below)
constexpr int MS_MAX_G = 16;       // at most 16^3 bins per shape
constexpr int MS_MAX_SIZE = 512;
constexpr int MS_PREP_T = 256;

__host__ __device__ inline int ms_bins(int S) {
  const int g = (S + MS_BIN_CELLS - 1) / MS_BIN_CELLS;
  return g > MS_MAX_G ? MS_MAX_G : g;
}

__device__ __forceinline__ double ms_lat(int i, int S) { return (2.0 * (double)i) / (double)S - 1.0; }

struct MsWs {
  int32_t* cnt;      // [batch * G3]      triangles per bin
  int32_t* off;      // [batch * G3 + 1]  exclusive scan
  int32_t* cursor;   // [batch * G3]      fill cursors
  int32_t* box;      // [batch * G3 * 6]  keys of min xyz, max xyz
  void* scan_ws;
  float* tri;        // [total_faces * 9] coordinates in bin order (last: the only array sized by the faces)
};

inline size_t ms_align(size_t b) { return (b + 255) & ~(size_t)255; }

size_t ms_layout(int batch, int64_t total_faces, int S, char* base, MsWs* w) {
  const int G = ms_bins(S);
  const int64_t nb = (int64_t)batch * G * G * G;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += ms_align(bytes);
    return p;
  };
  MsWs l;
  l.cnt = (int32_t*)take(nb * sizeof(int32_t));
  l.off = (int32_t*)take((nb + 1) * sizeof(int32_t));
  l.cursor = (int32_t*)take(nb * sizeof(int32_t));
  l.box = (int32_t*)take(nb * 6 * sizeof(int32_t));
  l.scan_ws = take(ofx_scan_ws_bytes(nb));
  l.tri = (float*)take((size_t)total_faces * 9 * sizeof(float));
  if (w) *w = l;
  return o;
}

struct MsMesh {
  const float* verts;
  const int32_t* faces;
  const int64_t* vert_off;
  const int64_t* tri_off;
  int batch, S, G;
};

__device__ __forceinline__ int ms_bin_of(const MsMesh& m, const float (&c)[9]) {
  int g[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double mid = ((double)c[a] + (double)c[3 + a] + (double)c[6 + a]) * (1.0 / 3.0);
    double f = floor((mid + 1.0) * 0.5 * (double)m.G);
    f = f < 0.0 ? 0.0 : f;
    f = f > (double)(m.G - 1) ? (double)(m.G - 1) : f;
    g[a] = (int)f;
  }
  return (g[0] * m.G + g[1]) * m.G + g[2];
}

__global__ __launch_bounds__(MS_PREP_T) void ms_init_kernel(int64_t nb, int32_t* __restrict__ cnt,
                                                            int32_t* __restrict__ cursor, int32_t* __restrict__ box,
                                                            int batch, int32_t* __restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * MS_PREP_T;
  for (int64_t i = (int64_t)blockIdx.x * MS_PREP_T + threadIdx.x; i < nb; i += stride) {
    cnt[i] = 0;
    cursor[i] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      box[i * 6 + a] = INT32_MAX;
      box[i * 6 + 3 + a] = INT32_MIN;
    }
    if (i < batch) status[i] = 0;
  }
}

// fill == 0: validate, count and bound; fill == 1: copy the coordinates into bin order.
template <int FILL>
__global__ __launch_bounds__(MS_PREP_T) void ms_bin_kernel(MsMesh m, MsWs w, int32_t* __restrict__ status) {
  const int64_t total = m.tri_off[m.batch];
  const int64_t stride = (int64_t)gridDim.x * MS_PREP_T;
  const int G3 = m.G * m.G * m.G;
  for (int64_t t = (int64_t)blockIdx.x * MS_PREP_T + threadIdx.x; t < total; t += stride) {
    const int b = ms_shape_of(m.tri_off, m.batch, t);
    float c[9];
    if (!ms_load(m.verts, m.faces, m.vert_off, t, b, c)) {
      if (!FILL) atomicOr(&status[b], 1);
      continue;
    }
    const int64_t bin = (int64_t)b * G3 + ms_bin_of(m, c);
    if (!FILL) {
      atomicAdd(&w.cnt[bin], 1);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        atomicMin(&w.box[bin * 6 + a], ms_key(fminf(fminf(c[a], c[3 + a]), c[6 + a])));
        atomicMax(&w.box[bin * 6 + 3 + a], ms_key(fmaxf(fmaxf(c[a], c[3 + a]), c[6 + a])));
      }
    } else {
      const int64_t slot = (int64_t)w.off[bin] + atomicAdd(&w.cursor[bin], 1);
#pragma unroll
      for (int k = 0; k < 9; ++k) w.tri[slot * 9 + k] = c[k];
    }
  }
}

template <bool COUNT>
__global__ __launch_bounds__(MS_T) void ms_dist_kernel(int S, int G, MsWs w, const int32_t* __restrict__ status,
                                                       float* __restrict__ sdf, unsigned long long* counters) {
  __shared__ double rec[MS_REC * MS_T];
  uint32_t tally[3] = {0u, 0u, 0u};            // bins searched, triangles staged, triangles evaluated (per brick)
  const int b = blockIdx.y;
  if (status[b]) return;
  const int lane = threadIdx.x;
  const int NB = (S + MS_BRICK - 1) / MS_BRICK;
  int r = blockIdx.x;
  const int bz = r % NB;
  r /= NB;
  const int by = r % NB, bx = r / NB;
  const int brick[3] = {bx, by, bz};
  const int own[3] = {lane >> 4, (lane >> 2) & 3, lane & 3};
  int idx[3];
  double p[3];
  float klo[3], khi[3];
  bool live = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int first = brick[a] * MS_BRICK;
    const int last = min(first + MS_BRICK - 1, S - 1);
    idx[a] = first + own[a];
    live = live && idx[a] < S;
    p[a] = ms_lat(min(idx[a], S - 1), S);       // a lane past the lattice repeats its last point and writes nothing
    klo[a] = (float)ms_lat(first, S);
    khi[a] = (float)ms_lat(last, S);
  }
  const int G3 = G * G * G;
  const int64_t bin0 = (int64_t)b * G3;

  // pass 1: the smallest of the bins' largest distances, and the bin that gives it (ties: the lowest bin)
  float u_best = INFINITY;
  int u_bin = -1;
  for (int g = lane; g < G3; g += MS_T) {
    if (w.off[bin0 + g + 1] - w.off[bin0 + g] <= 0) continue;
    float lo[3], hi[3];
    ms_bin_box(w.box, bin0 + g, lo, hi);
    const float u = ms_box_max2(klo, khi, lo, hi);
    if (u_bin < 0 || u < u_best) {          // a bin is chosen even if its distance overflows fp32
      u_best = u;
      u_bin = g;
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const float ou = __shfl_xor(u_best, s);
    const int ob = __shfl_xor(u_bin, s);
    if (ob >= 0 && (u_bin < 0 || ou < u_best || (ou == u_best && ob < u_bin))) {
      u_best = ou;
      u_bin = ob;
    }
  }
  if (u_bin < 0) return;                         // no valid triangle: the caller refuses such a shape
  const float upper = u_best * (1.f + MS_REL) + MS_ABS;

  double best = INFINITY;
  int32_t none = 0;                              // the lattice keeps no face
  ms_search_bin<COUNT, false>(w.tri, w.off[bin0 + u_bin], w.off[bin0 + u_bin + 1] - w.off[bin0 + u_bin], lane, klo, khi,
                              p, best, none, rec, nullptr, tally);

  // pass 2: every other bin that can still hold a nearer triangle
  for (int g0 = 0; g0 < G3; g0 += MS_T) {
    const int g = g0 + lane;
    bool cand = false;
    if (g < G3 && g != u_bin && w.off[bin0 + g + 1] - w.off[bin0 + g] > 0) {
      float lo[3], hi[3];
      ms_bin_box(w.box, bin0 + g, lo, hi);
      cand = !ms_beyond(ms_box_min2(klo, khi, lo, hi), upper);
    }
    uint64_t mask = __ballot(cand);
    while (mask) {
      const int j = __ffsll((unsigned long long)mask) - 1;
      mask &= mask - 1;
      const int64_t bin = bin0 + g0 + j;
      float lo[3], hi[3];
      ms_bin_box(w.box, bin, lo, hi);
      if (ms_beyond(ms_box_min2(klo, khi, lo, hi), ms_wave_max((float)best))) continue;
      ms_search_bin<COUNT, false>(w.tri, w.off[bin], w.off[bin + 1] - w.off[bin], lane, klo, khi, p, best, none, rec,
                                  nullptr, tally);
    }
  }
  if (live) sdf[(((int64_t)b * S + idx[0]) * S + idx[1]) * S + idx[2]] = (float)sqrt(best);
  if (COUNT && lane < 3) atomicAdd(&counters[lane], (unsigned long long)tally[lane]);
}

// ---- sign ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MS_T) void ms_sign_kernel(int S, int G, MsWs w, const int32_t* __restrict__ status,
                                                       float* __restrict__ sdf) {
  __shared__ double rec[MS_REC * MS_T];
  __shared__ uint32_t bits[(MS_MAX_SIZE / 32) * MS_T];
  const int b = blockIdx.y;
  if (status[b]) return;
  const int lane = threadIdx.x;
  const int NT = (S + MS_TILE - 1) / MS_TILE;
  const int tj = blockIdx.x / NT, tk = blockIdx.x % NT;
  const int j = tj * MS_TILE + (lane >> 3), k = tk * MS_TILE + (lane & 7);
  const bool live = j < S && k < S;
  const double py = ms_lat(min(j, S - 1), S), pz = ms_lat(min(k, S - 1), S);
  const double ylo = ms_lat(tj * MS_TILE, S), yhi = ms_lat(min(tj * MS_TILE + MS_TILE - 1, S - 1), S);
  const double zlo = ms_lat(tk * MS_TILE, S), zhi = ms_lat(min(tk * MS_TILE + MS_TILE - 1, S - 1), S);
  const int words = (S + 31) >> 5;
  for (int q = 0; q < words; ++q) bits[q * MS_T + lane] = 0u;
  const int G3 = G * G * G;
  const int64_t bin0 = (int64_t)b * G3;

  for (int g0 = 0; g0 < G3; g0 += MS_T) {
    const int g = g0 + lane;
    bool cand = false;
    if (g < G3 && w.off[bin0 + g + 1] - w.off[bin0 + g] > 0) {
      float lo[3], hi[3];
      ms_bin_box(w.box, bin0 + g, lo, hi);
      cand = (double)lo[1] <= yhi && (double)hi[1] >= ylo && (double)lo[2] <= zhi && (double)hi[2] >= zlo;
    }
    uint64_t bmask = __ballot(cand);
    while (bmask) {
      const int jb = __ffsll((unsigned long long)bmask) - 1;
      bmask &= bmask - 1;
      const int64_t start = w.off[bin0 + g0 + jb];
      const int count = w.off[bin0 + g0 + jb + 1] - (int32_t)start;
      for (int base = 0; base < count; base += MS_T) {
        const int t = base + lane;
        bool keep = t < count;
        if (keep) {
          float c[9];
#pragma unroll
          for (int q = 0; q < 9; ++q) c[q] = w.tri[(start + t) * 9 + q];
          const double y0 = c[1], z0 = c[2], y1 = c[4], z1 = c[5], y2 = c[7], z2 = c[8];
          keep = fmin(fmin(y0, y1), y2) <= yhi && fmax(fmax(y0, y1), y2) >= ylo &&
                 fmin(fmin(z0, z1), z2) <= zhi && fmax(fmax(z0, z1), z2) >= zlo;
          const double area = ms_proj_area(y0, z0, y1, z1, y2, z2);
          keep = keep && area != 0.0;           // a projection of zero area never counts
          if (keep) {
            rec[0 * MS_T + lane] = y0;
            rec[1 * MS_T + lane] = z0;
            rec[2 * MS_T + lane] = y1;
            rec[3 * MS_T + lane] = z1;
            rec[4 * MS_T + lane] = y2;
            rec[5 * MS_T + lane] = z2;
            rec[6 * MS_T + lane] = (double)c[0];
            rec[7 * MS_T + lane] = (double)c[3] - (double)c[0];
            rec[8 * MS_T + lane] = (double)c[6] - (double)c[0];
            rec[9 * MS_T + lane] = area;
          }
        }
        __syncthreads();
        uint64_t mask = __ballot(keep);
        while (mask) {
          const int q = __ffsll((unsigned long long)mask) - 1;
          mask &= mask - 1;
          const double y0 = rec[0 * MS_T + q], z0 = rec[1 * MS_T + q], y1 = rec[2 * MS_T + q], z1 = rec[3 * MS_T + q];
          const double y2 = rec[4 * MS_T + q], z2 = rec[5 * MS_T + q];
          int s0, s1, s2;
          const double e01 = ms_edge(y0, z0, y1, z1, py, pz, s0);     // weight of vertex 2
          ms_edge(y1, z1, y2, z2, py, pz, s1);
          const double e20 = ms_edge(y2, z2, y0, z0, py, pz, s2);     // weight of vertex 1
          if (s0 == s1 && s1 == s2) {
            const double x = ms_cross_x(rec, q, e01, e20);
            // the first lattice index whose x is not left of the crossing
            double f = ceil((x + 1.0) * 0.5 * (double)S);
            f = f < 0.0 ? 0.0 : (f > (double)S ? (double)S : f);
            int ci = (int)f;
            if (ci > 0 && ms_lat(ci - 1, S) >= x) --ci;
            if (ci < S && ms_lat(ci, S) < x) ++ci;
            if (ci < S) bits[(ci >> 5) * MS_T + lane] ^= 1u << (ci & 31);
          }
        }
        __syncthreads();
      }
    }
  }
  if (!live) return;
  uint32_t par = 0u, word = 0u;
  for (int i = 0; i < S; ++i) {
    if ((i & 31) == 0) word = bits[(i >> 5) * MS_T + lane];
    par ^= (word >> (i & 31)) & 1u;
    if (par) {
      float* v = sdf + (((int64_t)b * S + i) * S + j) * S + k;
      *v = -*v;
    }
  }
}

unsigned long long* ms_counters = nullptr;      // ofx_mesh_sdf_set_counters

bool ms_valid(int batch, int64_t total_verts, int64_t total_faces, int size) {
  return batch >= 1 && batch <= 65535 && total_verts >= 1 && total_faces >= 1 && total_faces <= INT32_MAX &&
         size >= 2 && size <= MS_MAX_SIZE;
}

}  // namespace

extern "C" size_t ofx_mesh_sdf_ws_bytes(int batch, int64_t total_verts, int64_t total_faces, int size) {
  if (!ms_valid(batch, total_verts, total_faces, size)) return 0;
  return ms_layout(batch, total_faces, size, nullptr, nullptr);
}

extern "C" int ofx_mesh_sdf_set_counters(unsigned long long* words) {
  ms_counters = words;
  return OFX_OK;
}

extern "C" int ofx_mesh_sdf(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                            int batch, int size, int signed_, float* sdf, void* ws, int32_t* status, void* stream) {
  if (!verts || !faces || !vert_off || !tri_off || !sdf || !ws || !status || !ms_valid(batch, 1, 1, size))
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  const int S = size, G = ms_bins(S);
  const int64_t nb = (int64_t)batch * G * G * G;
  MsWs w;
  ms_layout(batch, 0, S, (char*)ws, &w);          // the face-sized array is the last one: its size is not needed
  const MsMesh m{verts, faces, vert_off, tri_off, batch, S, G};
  ms_init_kernel<<<ofx_grid(nb, MS_PREP_T), MS_PREP_T, 0, st>>>(nb, w.cnt, w.cursor, w.box, batch, status);
  OFX_LAUNCH_CHECK();
  const int prep = 2048;                          // grid-stride: the face count lives on the device
  ms_bin_kernel<0><<<prep, MS_PREP_T, 0, st>>>(m, w, status);
  OFX_LAUNCH_CHECK();
  const int rc = ofx_scan_i32(w.cnt, w.off, nb, w.scan_ws, stream);
  if (rc) return rc;
  ms_bin_kernel<1><<<prep, MS_PREP_T, 0, st>>>(m, w, status);
  OFX_LAUNCH_CHECK();
  const int NB = (S + MS_BRICK - 1) / MS_BRICK;
  const dim3 bricks((unsigned)(NB * NB * NB), (unsigned)batch);
  if (ms_counters) ms_dist_kernel<true><<<bricks, MS_T, 0, st>>>(S, G, w, status, sdf, ms_counters);
  else ms_dist_kernel<false><<<bricks, MS_T, 0, st>>>(S, G, w, status, sdf, nullptr);
  OFX_LAUNCH_CHECK();
  if (signed_) {
    const int NT = (S + MS_TILE - 1) / MS_TILE;
    ms_sign_kernel<<<dim3((unsigned)(NT * NT), (unsigned)batch), MS_T, 0, st>>>(S, G, w, status, sdf);
    OFX_LAUNCH_CHECK();
  }
  return OFX_OK;
}

// Ray casting against triangle meshes: first hit, face, hit point and the cosine between the face normal and the ray,
// the sibling of the point queries of ofx_meshquery.hip.  Contract: include/ofx.h; tests/raycast_oracle.py restates it in
// float64 (brute force).  DESIGN.md section 4.20 has the exactness argument and the figures.
//
//   bins   the per-shape G^3 centroid bins of ofx_tribins.h, built by ofx_tribins_build: the structure the point
//          queries search (section 4.19).  Nothing below depends on which bin a triangle is in or on the order inside
//          a bin.
//   order  a key per ray: shape << 32 | invalid << 30 | 27-bit Morton code of the origin clamped into the shape's box
//          << 3 | octant of the direction; ofx_points_sort (stable) orders them, so a wave gets 64 neighbouring rays.
//          `coherent` != 0: the caller's order is kept (camera rays in 8 x 8 pixel tiles).  A performance device only.
//   cast   one wave per 64 consecutive rays of one shape.  The bins are visited slab by slab along the dominant axis of
//          the wave's first valid ray, front to back.  A lane takes part in a bin iff the fp32 slab test of the bin's
//          box, inflated by RC_REL, passes for its ray with an entry not beyond its running best; a bin no lane takes
//          part in is skipped (ballot).  Otherwise 64 triangles at a time are staged into LDS, field-major (fp32: the
//          conversion to fp64 is exact and is done in registers), every staged triangle's own box goes through the
//          same test, and the lanes that pass evaluate the pair.  best / face are updated by
//          t < best || (t == best && id < face): the minimum over ALL triangles of one fixed fp64 expression and the
//          lowest index among its ties, whatever was skipped.  Point and cosine are evaluated once at the end from the
//          winning face's original vertices.
//   scan   ofx_ray_scan: the hits of a cast, compacted in ray order (ballot + ofx_scan_i32 over block counts) into an
//          oriented point cloud, optionally with Gaussian noise along the ray from the counter hash.
#include "ofx_tribins.h"

#include <cmath>

#pragma clang fp contract(off)

#include "ofx_tri.h"

namespace {

constexpr float RC_REL = 1.0e-5f;  // every box is inflated by RC_REL * (largest |bound| + |origin|) per axis before a skip
constexpr float RC_DMIN = 0x1p-100f, RC_DMAX = 0x1p100f;      // a direction component outside: the ray is never culled

// the meshes of a call and its rays
struct RcMesh : TbMesh {
  const float* org;
  const float* dir;
  const int64_t* ray_off;
};

// A ray the cast answers: every component finite and a direction that is not zero.
__device__ __forceinline__ bool rc_valid(const float (&o)[3], const float (&d)[3]) {
  bool fin = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) fin = fin && isfinite(o[a]) && isfinite(d[a]);
  return fin && (d[0] != 0.f || d[1] != 0.f || d[2] != 0.f);
}

// Sort key of every ray.  Only the shape bits matter for the result (a shape's rays stay in its range of positions).
__global__ __launch_bounds__(TB_PREP_T) void rc_key_kernel(RcMesh m, TbBins w, TbOrder ord, int64_t total_q) {
  const int64_t stride = (int64_t)gridDim.x * TB_PREP_T;
  for (int64_t i = (int64_t)blockIdx.x * TB_PREP_T + threadIdx.x; i < total_q; i += stride) {
    const int b = ms_shape_of(m.ray_off, m.batch, i);
    float o[3], d[3];
    int cell[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      o[a] = m.org[i * 3 + a];
      d[a] = m.dir[i * 3 + a];
      const float lo = ms_unkey(w.sbox[b * 6 + a]), ext = ms_unkey(w.sbox[b * 6 + 3 + a]) - lo;
      const float f = (o[a] - lo) / ext * 512.f;
      cell[a] = f >= 0.f ? (f < 511.f ? (int)f : 511) : 0;      // a NaN lands in cell 0
    }
    const uint64_t oct = (d[0] < 0.f ? 4u : 0u) | (d[1] < 0.f ? 2u : 0u) | (d[2] < 0.f ? 1u : 0u);
    const uint64_t code = rc_valid(o, d) ? ((ofx_xyz2morton(cell[0], cell[1], cell[2]) << 3) | oct) : (1ull << 30);
    ord.key[i] = (int64_t)(((uint64_t)b << 32) | code);
    ord.idx[i] = (int32_t)i;
  }
}

// ---- the pair -----------------------------------------------------------------------------------------------------
__device__ __forceinline__ double rc_pick(double v0, double v1, double v2, int k) {
  return k == 0 ? v0 : (k == 1 ? v1 : v2);
}

// What the pair needs of a ray: the permutation (kz the dominant axis, the lowest index among equal |d|; kx, ky the
// other two, swapped where d[kz] < 0 so that the winding is kept), the origin and the shear constants.
struct RcRay {
  int kx, ky, kz;
  double o[3];               // the origin
  double sx, sy, sz;         // d[kx] / d[kz], d[ky] / d[kz], 1 / d[kz]
};

__device__ __forceinline__ RcRay rc_ray(const float (&o)[3], const float (&d)[3]) {
  RcRay r;
  const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
  int kz = ay > ax ? 1 : 0;
  kz = az > fmaxf(ax, ay) ? 2 : kz;
  int kx = kz == 2 ? 0 : kz + 1, ky = kx == 2 ? 0 : kx + 1;
  const double dz = rc_pick((double)d[0], (double)d[1], (double)d[2], kz);
  if (dz < 0.0) {
    const int s = kx;
    kx = ky;
    ky = s;
  }
  r.kx = kx;
  r.ky = ky;
  r.kz = kz;
#pragma unroll
  for (int a = 0; a < 3; ++a) r.o[a] = (double)o[a];
  r.sx = rc_pick((double)d[0], (double)d[1], (double)d[2], kx) / dz;
  r.sy = rc_pick((double)d[0], (double)d[1], (double)d[2], ky) / dz;
  r.sz = 1.0 / dz;
  return r;
}

// One vertex seen from the ray: its sheared coordinates (x, y) and its parameter z along the ray.  One expression per
// (ray, vertex): two triangles that share a vertex see the same point.
__device__ __forceinline__ void rc_vertex(const RcRay& r, float v0, float v1, float v2, double& x, double& y,
                                          double& z) {
  const double a0 = (double)v0 - r.o[0], a1 = (double)v1 - r.o[1], a2 = (double)v2 - r.o[2];
  const double ax = rc_pick(a0, a1, a2, r.kx), ay = rc_pick(a0, a1, a2, r.ky), az = rc_pick(a0, a1, a2, r.kz);
  x = ax - r.sx * az;
  y = ay - r.sy * az;
  z = r.sz * az;
}

// The three edge functions of triangle c (nine coordinates) at the ray and the parameters of its corners; true iff the
// ray meets the triangle (two-sided; a triangle seen edge-on or of zero area never).  Then t = the parameter of the hit.
__device__ __forceinline__ bool rc_pair(const RcRay& r, const float (&c)[9], double& u, double& v, double& w,
                                        double& det, double& t) {
  double ax, ay, az, bx, by, bz, cx, cy, cz;
  rc_vertex(r, c[0], c[1], c[2], ax, ay, az);
  rc_vertex(r, c[3], c[4], c[5], bx, by, bz);
  rc_vertex(r, c[6], c[7], c[8], cx, cy, cz);
  u = ms_det2(cx, by, cy, bx);
  v = ms_det2(ax, cy, ay, cx);
  w = ms_det2(bx, ay, by, ax);
  if (!((u >= 0.0 && v >= 0.0 && w >= 0.0) || (u <= 0.0 && v <= 0.0 && w <= 0.0))) return false;
  det = (u + v) + w;
  if (det == 0.0) return false;
  t = ((u * az + v * bz) + w * cz) / det;
  return true;
}

// ---- the search ---------------------------------------------------------------------------------------------------
// fp32 slab test of the box [lo, hi] inflated by RC_REL * (largest |bound| + |origin|) on every axis: false only if the
// ray certainly has no hit with tmin <= (float)t <= tmax on a triangle inside the box; `entry` is then a lower bound
// of every such t.  inv = 1 / d (inf for a zero component: fminf / fmaxf drop the NaN of 0 * inf, which arises only for
// an origin on the inflated bound).
__device__ __forceinline__ bool rc_slab(const float (&o)[3], const float (&inv)[3], const float (&lo)[3],
                                        const float (&hi)[3], float tmin, float tmax, float& entry) {
  float tn = -INFINITY, tf = INFINITY;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float mg = RC_REL * (fmaxf(fabsf(lo[a]), fabsf(hi[a])) + fabsf(o[a]));
    const float t1 = ((lo[a] - mg) - o[a]) * inv[a], t2 = ((hi[a] + mg) - o[a]) * inv[a];
    tn = fmaxf(tn, fminf(t1, t2));
    tf = fminf(tf, fmaxf(t1, t2));
  }
  entry = tn;
  return tn <= tf && tn <= tmax && tf >= tmin;
}

template <bool COUNT>
__global__ __launch_bounds__(MS_T) void rc_cast_kernel(RcMesh m, TbBins ws, const int32_t* __restrict__ order,
                                                       const int32_t* __restrict__ status, float tmin, float tmax,
                                                       float* __restrict__ t_out, int32_t* __restrict__ face_out,
                                                       float* __restrict__ point, float* __restrict__ cosn,
                                                       unsigned long long* counters) {
  __shared__ float rec[9 * MS_T];
  __shared__ int32_t ids[MS_T];
  uint32_t tally[3] = {0u, 0u, 0u};            // bins visited, triangles staged, pairs evaluated (per wave)
  const int b = blockIdx.y;
  if (status[b]) return;
  const int64_t q0 = m.ray_off[b], nq = m.ray_off[b + 1] - q0;
  if ((int64_t)blockIdx.x * MS_T >= nq) return;
  const int lane = threadIdx.x;
  const int64_t s = (int64_t)blockIdx.x * MS_T + lane;
  const int64_t qi = s < nq ? (order ? (int64_t)order[q0 + s] : q0 + s) : -1;
  float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 1.f};
  if (qi >= 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      o[a] = m.org[qi * 3 + a];
      d[a] = m.dir[qi * 3 + a];
    }
  }
  const bool act = qi >= 0 && rc_valid(o, d);
  if (qi >= 0 && !act) {                        // a non-finite or zero-direction ray: inf, -1, NaN, NaN
    t_out[qi] = INFINITY;
    face_out[qi] = -1;
    if (point) point[qi * 3] = point[qi * 3 + 1] = point[qi * 3 + 2] = NAN;
    if (cosn) cosn[qi] = NAN;
  }
  if (!act) {                                   // a lane without a ray casts a harmless one and writes nothing
    o[0] = o[1] = o[2] = 0.f;
    d[0] = d[1] = 0.f;
    d[2] = 1.f;
  }
  const uint64_t acts = __ballot(act);
  if (acts == 0ull) return;
  const RcRay r = rc_ray(o, d);
  float inv[3];
  bool wild = false;                            // a component too small or too large for 1 / d in fp32: never culled
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    inv[a] = 1.f / d[a];
    wild = wild || (d[a] != 0.f && !(fabsf(d[a]) >= RC_DMIN && fabsf(d[a]) <= RC_DMAX));
  }
  // front to back: the slabs of the grid along the dominant axis of the first valid ray, in its direction
  const int lead = __ffsll((unsigned long long)acts) - 1;
  const int wk = __shfl(r.kz, lead);
  const bool wneg = __shfl((int)(rc_pick((double)d[0], (double)d[1], (double)d[2], r.kz) < 0.0), lead) != 0;
  const int G = tb_G(m, b), G2 = G * G;
  const int64_t bin0 = (int64_t)b * m.GS;
  double best = INFINITY;
  int32_t bf = INT32_MAX;

  for (int sl = 0; sl < G; ++sl) {
    const int c = wneg ? G - 1 - sl : sl;
    for (int p0 = 0; p0 < G2; p0 += MS_T) {
      const int p = p0 + lane;
      int g = 0;
      bool some = false;
      float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
      if (p < G2) {
        const int e = p / G, f = p - e * G;
        g = wk == 0 ? (c * G + e) * G + f : (wk == 1 ? (e * G + c) * G + f : (e * G + f) * G + c);
        some = ws.off[bin0 + g + 1] - ws.off[bin0 + g] > 0;
        if (some) ms_bin_box(ws.box, bin0 + g, lo, hi);
      }
      uint64_t bmask = __ballot(some);
      while (bmask) {
        const int jb = __ffsll((unsigned long long)bmask) - 1;
        bmask &= bmask - 1;
        float blo[3], bhi[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          blo[a] = __shfl(lo[a], jb);
          bhi[a] = __shfl(hi[a], jb);
        }
        float entry;
        const bool in = act && (wild || (rc_slab(o, inv, blo, bhi, tmin, tmax, entry) && !((double)entry > best)));
        if (__ballot(in) == 0ull) continue;
        const int64_t bin = bin0 + __shfl(g, jb);
        const int64_t start = ws.off[bin];
        const int count = ws.off[bin + 1] - (int32_t)start;
        if (COUNT) {
          tally[0] += 1u;
          tally[1] += (uint32_t)count;
        }
        for (int base = 0; base < count; base += MS_T) {
          const int n = count - base < MS_T ? count - base : MS_T;
          if (lane < n) {
#pragma unroll
            for (int k = 0; k < 9; ++k) rec[k * MS_T + lane] = ws.tri[(start + base + lane) * TB_W + k];
            ids[lane] = __float_as_int(ws.tri[(start + base + lane) * TB_W + 9]);
          }
          __syncthreads();
          for (int j = 0; j < n; ++j) {
            float cc[9], tlo[3], thi[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) cc[k] = rec[k * MS_T + j];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
              tlo[a] = fminf(fminf(cc[a], cc[3 + a]), cc[6 + a]);
              thi[a] = fmaxf(fmaxf(cc[a], cc[3 + a]), cc[6 + a]);
            }
            const bool on = act && (wild || (rc_slab(o, inv, tlo, thi, tmin, tmax, entry) && !((double)entry > best)));
            const uint64_t ons = __ballot(on);
            if (ons == 0ull) continue;
            if (COUNT) tally[2] += (uint32_t)__popcll(ons);
            if (on) {
              double u, v, w, det, t;
              if (rc_pair(r, cc, u, v, w, det, t)) {
                const float tf = (float)t;
                const int32_t id = ids[j];
                if (tf >= tmin && tf <= tmax && tf < INFINITY && (t < best || (t == best && id < bf))) {
                  best = t;
                  bf = id;
                }
              }
            }
          }
          __syncthreads();
        }
      }
    }
  }
  if (act) {
    const bool hit = bf != INT32_MAX;
    t_out[qi] = hit ? (float)best : INFINITY;
    face_out[qi] = hit ? bf : -1;
    double pt[3] = {NAN, NAN, NAN}, cs = NAN;
    if (hit && (point || cosn)) {
      // the winning face again, from its original vertices (valid: the shape's status is 0)
      const int64_t tr = m.tri_off[b] + bf, v0 = m.vert_off[b];
      float cc[9];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int64_t vi = v0 + m.faces[tr * 3 + k];
#pragma unroll
        for (int a = 0; a < 3; ++a) cc[k * 3 + a] = m.verts[vi * 3 + a];
      }
      double u, v, w, det, t;
      if (rc_pair(r, cc, u, v, w, det, t)) {      // the pair that won, bit for bit
#pragma unroll
        for (int a = 0; a < 3; ++a)
          pt[a] = ((u * (double)cc[a] + v * (double)cc[3 + a]) + w * (double)cc[6 + a]) / det;
      }
      double ab[3], ac[3], nn[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        ab[a] = (double)cc[3 + a] - (double)cc[a];
        ac[a] = (double)cc[6 + a] - (double)cc[a];
      }
      ms_cross(ab, ac, nn);
      const double dd[3] = {(double)d[0], (double)d[1], (double)d[2]};
      cs = ms_dot(nn, dd) / (sqrt(ms_dot(nn, nn)) * sqrt(ms_dot(dd, dd)));
    }
    if (point) {
#pragma unroll
      for (int a = 0; a < 3; ++a) point[qi * 3 + a] = (float)pt[a];
    }
    if (cosn) cosn[qi] = (float)cs;
  }
  if (COUNT && lane < 3) atomicAdd(&counters[lane], (unsigned long long)tally[lane]);
}

// ---- the scan -----------------------------------------------------------------------------------------------------
constexpr int RS_T = 256;

__global__ __launch_bounds__(RS_T) void rs_count_kernel(const int32_t* __restrict__ face, int64_t total_q,
                                                        int32_t* __restrict__ blk) {
  __shared__ int32_t part[RS_T / MS_T];
  const int64_t i = (int64_t)blockIdx.x * RS_T + threadIdx.x;
  const uint64_t hits = __ballot(i < total_q && face[i] >= 0);
  if ((threadIdx.x & (MS_T - 1)) == 0) part[threadIdx.x / MS_T] = __popcll(hits);
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t n = 0;
#pragma unroll
    for (int k = 0; k < RS_T / MS_T; ++k) n += part[k];
    blk[blockIdx.x] = n;
  }
}

// standard normal from two draws of the counter hash (Box-Muller, fp64)
__device__ __forceinline__ double rs_normal(uint64_t seed, int64_t shape, int64_t ray) {
  const uint64_t h = mt_step(mt_step(seed, (uint64_t)shape), (uint64_t)ray);
  const double u1 = ((double)(mt_step(h, 0) >> 11) + 1.0) * 0x1p-53;        // (0, 1]
  const double u2 = (double)(mt_step(h, 1) >> 11) * 0x1p-53;               // [0, 1)
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

__global__ __launch_bounds__(RS_T) void rs_fill_kernel(RcMesh m, const float* __restrict__ t,
                                                       const int32_t* __restrict__ face, int64_t total_q,
                                                       const int32_t* __restrict__ blk_off, float sigma, uint64_t seed,
                                                       float* __restrict__ points, float* __restrict__ normals) {
  __shared__ int32_t part[RS_T / MS_T];
  const int64_t i = (int64_t)blockIdx.x * RS_T + threadIdx.x;
  const bool hit = i < total_q && face[i] >= 0;
  const uint64_t hits = __ballot(hit);
  const int lane = threadIdx.x & (MS_T - 1), wv = threadIdx.x / MS_T;
  if (lane == 0) part[wv] = __popcll(hits);
  __syncthreads();
  if (!hit) return;
  int64_t slot = blk_off[blockIdx.x] + __popcll(hits & ((1ull << lane) - 1ull));
  for (int k = 0; k < wv; ++k) slot += part[k];
  const int b = ms_shape_of(m.ray_off, m.batch, i);
  const int64_t tr = m.tri_off[b] + face[i], v0 = m.vert_off[b], nv = m.vert_off[b + 1] - v0;
  double c[9];
  bool ok = tr < m.tri_off[b + 1];               // a face or vertex index out of range: NaN, nothing read through it
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t id = ok ? (int64_t)m.faces[tr * 3 + k] : -1;
    ok = ok && id >= 0 && id < nv;
#pragma unroll
    for (int a = 0; a < 3; ++a) c[k * 3 + a] = ok ? (double)m.verts[(v0 + id) * 3 + a] : NAN;
  }
  double ab[3], ac[3], nn[3], dd[3], oo[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ab[a] = c[3 + a] - c[a];
    ac[a] = c[6 + a] - c[a];
    dd[a] = (double)m.dir[i * 3 + a];
    oo[a] = (double)m.org[i * 3 + a];
  }
  ms_cross(ab, ac, nn);
  const double len = sqrt(ms_dot(nn, nn));
  const double flip = ms_dot(nn, dd) > 0.0 ? -1.0 : 1.0;        // towards the camera: against the ray
  double along = (double)t[i];
  if (sigma > 0.f) along = along + ((double)sigma * rs_normal(seed, b, i - m.ray_off[b])) / sqrt(ms_dot(dd, dd));
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    points[slot * 3 + a] = (float)(oo[a] + along * dd[a]);
    normals[slot * 3 + a] = (float)((flip * nn[a]) / len);
  }
}

// where each shape's points begin in the compacted arrays: the hits before its first ray; the last entry the total
__global__ void rs_offsets_kernel(const int64_t* __restrict__ ray_off, int batch, const int32_t* __restrict__ face,
                                  int64_t total_q, const int32_t* __restrict__ blk_off, int64_t nblk,
                                  int64_t* __restrict__ out_off) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b > batch) return;
  const int64_t i = ray_off[b];
  if (i >= total_q) {
    out_off[b] = blk_off[nblk];
    return;
  }
  const int64_t k = i / RS_T;
  int64_t n = blk_off[k];
  for (int64_t j = k * RS_T; j < i; ++j) n += face[j] >= 0 ? 1 : 0;
  out_off[b] = n;
}

unsigned long long* rc_counters = nullptr;      // ofx_ray_cast_set_counters

inline size_t rs_layout(int64_t total_q, char* base, int32_t** blk, int32_t** blk_off, void** scan_ws) {
  const int64_t nblk = ofx_cdiv(total_q > 0 ? total_q : 1, RS_T);
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + o : nullptr;
    o += tb_align(bytes);
    return p;
  };
  int32_t* a = (int32_t*)take(nblk * sizeof(int32_t));
  int32_t* c = (int32_t*)take((nblk + 1) * sizeof(int32_t));
  void* s = take(ofx_scan_ws_bytes(nblk));
  if (blk) *blk = a;
  if (blk_off) *blk_off = c;
  if (scan_ws) *scan_ws = s;
  return o;
}

}  // namespace

extern "C" size_t ofx_ray_cast_ws_bytes(int batch, int64_t total_verts, int64_t total_faces, int64_t total_q,
                                        int bins) {
  if (!ofx_tribins_args_ok(batch, total_verts, total_faces, total_q, bins)) return 0;
  return ofx_tribins_layout(batch, total_faces, total_q, bins, nullptr, nullptr, nullptr);
}

extern "C" int ofx_ray_cast_set_counters(unsigned long long* words) {
  rc_counters = words;
  return OFX_OK;
}

extern "C" int ofx_ray_cast(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                            const float* org, const float* dir, const int64_t* ray_off, int batch, int64_t total_q,
                            int64_t max_q, float tmin, float tmax, int bins, int coherent, float* t, int32_t* face,
                            float* point, float* cosn, void* ws, int32_t* status, void* stream) {
  if (!verts || !faces || !vert_off || !tri_off || !ray_off || !ws || !status ||
      !ofx_tribins_args_ok(batch, 1, 1, total_q, bins) || max_q < 0 || max_q > total_q || tmin != tmin || tmax != tmax ||
      (total_q > 0 && (!org || !dir || !t || !face || max_q < 1)))
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  TbBins w;
  TbOrder o;
  ofx_tribins_layout(batch, 0, total_q, bins, (char*)ws, &w, &o);   // the records are last: their size is not needed
  const RcMesh m{{verts, faces, vert_off, tri_off, batch, bins, tb_stride(bins)}, org, dir, ray_off};
  int rc = ofx_tribins_build(m, w, total_q, status, stream);
  if (rc || total_q == 0) return rc;              // no rays: the status words are still written
  const int32_t* order = nullptr;
  if (!coherent) {
    rc_key_kernel<<<ofx_grid(total_q, TB_PREP_T), TB_PREP_T, 0, st>>>(m, w, o, total_q);
    OFX_LAUNCH_CHECK();
    rc = ofx_points_sort(o.key, o.idx, total_q, o.skey, o.sidx, o.sort_ws, o.sort_bytes, stream);
    if (rc) return rc;
    order = o.sidx;
  }
  const dim3 waves((unsigned)ofx_cdiv(max_q, MS_T), (unsigned)batch);
  if (rc_counters)
    rc_cast_kernel<true><<<waves, MS_T, 0, st>>>(m, w, order, status, tmin, tmax, t, face, point, cosn, rc_counters);
  else
    rc_cast_kernel<false><<<waves, MS_T, 0, st>>>(m, w, order, status, tmin, tmax, t, face, point, cosn, nullptr);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" size_t ofx_ray_scan_ws_bytes(int64_t total_q) {
  if (total_q < 0 || total_q > (int64_t(1) << 30)) return 0;
  return rs_layout(total_q, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int ofx_ray_scan(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                            const float* org, const float* dir, const int64_t* ray_off, int batch, int64_t total_q,
                            const float* t, const int32_t* face, float sigma, uint64_t seed, float* points,
                            float* normals, int64_t* out_off, void* ws, void* stream) {
  if (!verts || !faces || !vert_off || !tri_off || !ray_off || !out_off || !ws || batch < 1 || batch > 65535 ||
      total_q < 0 || total_q > (int64_t(1) << 30) || !(sigma >= 0.f) ||
      (total_q > 0 && (!org || !dir || !t || !face || !points || !normals)))
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  int32_t *blk, *blk_off;
  void* scan_ws;
  rs_layout(total_q, (char*)ws, &blk, &blk_off, &scan_ws);
  const int64_t nblk = ofx_cdiv(total_q > 0 ? total_q : 1, RS_T);
  const RcMesh m{{verts, faces, vert_off, tri_off, batch, 0, 0}, org, dir, ray_off};
  rs_count_kernel<<<(unsigned)nblk, RS_T, 0, st>>>(face, total_q, blk);
  OFX_LAUNCH_CHECK();
  const int rc = ofx_scan_i32(blk, blk_off, nblk, scan_ws, stream);
  if (rc) return rc;
  if (total_q > 0) {
    rs_fill_kernel<<<(unsigned)nblk, RS_T, 0, st>>>(m, t, face, total_q, blk_off, sigma, seed, points, normals);
    OFX_LAUNCH_CHECK();
  }
  rs_offsets_kernel<<<(unsigned)ofx_cdiv(batch + 1, RS_T), RS_T, 0, st>>>(ray_off, batch, face, total_q, blk_off, nblk,
                                                                          out_off);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

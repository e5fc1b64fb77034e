// Shaded views of triangle meshes (include/ofx.h, "rendering"): project -> raster -> shade.
//
//   project  one block per mesh reduces the bounding box and the largest distance from its centre (min / max only: the
//            result does not depend on order); one thread per (view, vertex) writes the screen position snapped to
//            1/256 pixel and the window depth.
//   raster   a 64-bit key per sample, (depth quantised to 32 bits) << 32 | triangle id, resolved with atomicMin.
//            Coverage is an integer function of the snapped coordinates (int64 edge functions at the sample
//            positions, top-left rule); depth is float64 in individually rounded operations.  Small path: a thread
//            per (view, triangle) walks the clamped pixel box; triangles whose box holds more than big_px pixels are
//            compacted with ballots into a list and rasterised one wave each.
//   shade    per pixel, from the winning triangles of its samples: flat two-sided glTF metallic-roughness shading
//            under three lights at the camera, in float64, once per distinct face at the pixel-centre ray; the
//            samples' colours are averaged in float64 and quantised once.
//
// 1, 4 or 16 samples per pixel (rd_sample: the one table).  The kernels are templates over the sample count; the
// one-sample entry points are their S = 1 instances, where a pixel's only sample is its centre.
//
// tests/render_oracle.py restates every stage; all float64 arithmetic here is uncontracted and in the oracle's order.
#include <float.h>

#include "ofx_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int RD_T = 256;                 // threads of the per-element kernels
constexpr int RD_NORM_T = 1024;           // threads of the per-mesh reduction
constexpr int RD_SUB = 256;               // sub-pixel units per pixel
constexpr int RD_HALF = 128;              // the pixel centre
constexpr double RD_GUARD = 67108864.0;   // 2^26 sub-pixel units
constexpr int32_t RD_DROPPED = INT32_MIN; // sx of a vertex whose triangles are dropped
constexpr int RD_BIG_BLOCKS = 1024;       // blocks of the large path (4 waves each)
constexpr uint64_t RD_EMPTY = ~0ull;

// ---- sample positions: sub-pixel units from the pixel's origin (256 i, 256 j) --------------------------------------
// 4: the rotated grid; 16: 128 + 16 o, one sample in every one of the pixel's 16 columns and 16 rows
__host__ __device__ constexpr int rd_sample(int samples, int s, int axis) {
  constexpr int g4[4][2] = {{96, 32}, {224, 96}, {32, 160}, {160, 224}};
  constexpr int o16[16][2] = {{1, 1}, {-1, -3}, {-3, 2}, {4, -1}, {-5, -2}, {2, 5}, {5, 3}, {3, -5},
                              {-2, 6}, {0, -7}, {-4, -6}, {-6, 4}, {-8, 0}, {7, -4}, {6, 7}, {-7, -8}};
  return samples == 4 ? g4[s][axis] : samples == 16 ? RD_HALF + 16 * o16[s][axis] : RD_HALF;
}
__host__ __device__ constexpr int rd_sample_min(int samples) { return samples == 4 ? 32 : samples == 16 ? 0 : RD_HALF; }
__host__ __device__ constexpr int rd_sample_max(int samples) {
  return samples == 4 ? 224 : samples == 16 ? 240 : RD_HALF;
}

// ---- normalisation: centre of the bounding box, largest distance from it (scale_to_unit_sphere) --------------------
__global__ __launch_bounds__(RD_NORM_T) void rd_norm_kernel(const float* __restrict__ verts,
                                                            const int64_t* __restrict__ offs, int batch, int normalize,
                                                            double* __restrict__ norm) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (!normalize) {
    if (tid < 4) norm[b * 4 + tid] = tid == 3 ? 1.0 : 0.0;
    return;
  }
  __shared__ double red[RD_NORM_T / 64][6];
  __shared__ double ctr[3];
  const int64_t v0 = offs[b], nv = offs[batch + b];
  const float* V = verts + v0 * 3;
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int64_t i = tid; i < nv; i += RD_NORM_T) {
    const float x = V[i * 3], y = V[i * 3 + 1], z = V[i * 3 + 2];
    if (!(fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX)) continue;   // non-finite: not in the box
    mn[0] = fminf(mn[0], x); mx[0] = fmaxf(mx[0], x);
    mn[1] = fminf(mn[1], y); mx[1] = fmaxf(mx[1], y);
    mn[2] = fminf(mn[2], z); mx[2] = fmaxf(mx[2], z);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], o));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o));
    }
  if ((tid & 63) == 0)
    for (int a = 0; a < 3; ++a) {
      red[tid >> 6][a] = mn[a];
      red[tid >> 6][3 + a] = mx[a];
    }
  __syncthreads();
  if (tid < 3) {
    double lo = red[0][tid], hi = red[0][3 + tid];
    for (int w = 1; w < RD_NORM_T / 64; ++w) {
      lo = fmin(lo, red[w][tid]);
      hi = fmax(hi, red[w][3 + tid]);
    }
    ctr[tid] = lo <= hi ? (lo + hi) * 0.5 : 0.0;       // no finite vertex: centre 0
  }
  __syncthreads();
  const double cx = ctr[0], cy = ctr[1], cz = ctr[2];
  double m = 0.0;
  for (int64_t i = tid; i < nv; i += RD_NORM_T) {
    const float x = V[i * 3], y = V[i * 3 + 1], z = V[i * 3 + 2];
    if (!(fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX)) continue;
    const double dx = (double)x - cx, dy = (double)y - cy, dz = (double)z - cz;
    m = fmax(m, (dx * dx + dy * dy) + dz * dz);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6][0] = m;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < RD_NORM_T / 64; ++w) m = fmax(m, red[w][0]);
    norm[b * 4 + 0] = cx;
    norm[b * 4 + 1] = cy;
    norm[b * 4 + 2] = cz;
    norm[b * 4 + 3] = m > 0.0 ? sqrt(m) : 1.0;         // a single point: scale 1
  }
}

// ---- projection: grid (vertex blocks, mesh, view) ------------------------------------------------------------------
// cam [views, 24] float64: 0..11 the view matrix (world -> camera, 3 x 4 row-major), 12..23 the pose (camera -> world)
__global__ __launch_bounds__(RD_T) void rd_project_kernel(const float* __restrict__ verts,
                                                          const int64_t* __restrict__ offs, int batch,
                                                          int64_t total_verts, const double* __restrict__ cam,
                                                          const double* __restrict__ norm, double focal,
                                                          double half_units, double znear, double dep_a, double dep_b,
                                                          int32_t* __restrict__ sxy, double* __restrict__ depth) {
  const int b = blockIdx.y, view = blockIdx.z;
  const int64_t i = (int64_t)blockIdx.x * RD_T + threadIdx.x;
  if (i >= offs[batch + b]) return;
  const int64_t g = offs[b] + i;
  const double* M = cam + (int64_t)view * 24;
  const double s = norm[b * 4 + 3];
  const double px = ((double)verts[g * 3] - norm[b * 4]) / s;
  const double py = ((double)verts[g * 3 + 1] - norm[b * 4 + 1]) / s;
  const double pz = ((double)verts[g * 3 + 2] - norm[b * 4 + 2]) / s;
  const double xe = ((M[0] * px + M[1] * py) + M[2] * pz) + M[3];
  const double ye = ((M[4] * px + M[5] * py) + M[6] * pz) + M[7];
  const double ze = ((M[8] * px + M[9] * py) + M[10] * pz) + M[11];
  const double w = -ze;
  const double fx = ((xe * focal) / w + 1.0) * half_units;     // sub-pixel units, x right
  const double fy = (1.0 - (ye * focal) / w) * half_units;     // row 0 is the top
  const double d = dep_a - dep_b / w;                          // window depth in [0, 1], affine in screen space
  // every comparison is written so that a NaN fails it
  const bool ok = w >= znear && fabs(fx) <= RD_GUARD && fabs(fy) <= RD_GUARD && fabs(d) <= DBL_MAX;
  const int64_t o = (int64_t)view * total_verts + g;
  sxy[o * 2] = ok ? (int32_t)rint(fx) : RD_DROPPED;
  sxy[o * 2 + 1] = ok ? (int32_t)rint(fy) : 0;
  depth[o] = ok ? d : 0.0;
}

// ---- the rasteriser's integer core ---------------------------------------------------------------------------------
struct RdTri {
  int64_t ax, ay, bx, by, cx, cy;   // snapped, oriented so that area2 > 0
  double za, zb, zc;
  int64_t area2;
  int x0, y0, x1, y1;               // pixel box, clamped to the screen, inclusive; empty if x0 > x1 or y0 > y1
};

__device__ __forceinline__ int64_t rd_edge(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py) {
  return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}
// an edge a -> b of a triangle with area2 > 0 owns the pixel centres on it iff it is a left edge or a top edge
__device__ __forceinline__ bool rd_owns(int64_t ax, int64_t ay, int64_t bx, int64_t by) {
  return by < ay || (by == ay && bx > ax);
}
__device__ __forceinline__ int rd_floor_div256(int64_t v) { return (int)(v >> 8); }   // arithmetic shift = floor

// 0: fine, 1: dropped, 2: zero area
template <int S>
__device__ __forceinline__ int rd_setup(const int32_t* __restrict__ sxy, const double* __restrict__ depth, int64_t ia,
                                        int64_t ib, int64_t ic, int size, RdTri& t) {
  const int2 a = *reinterpret_cast<const int2*>(sxy + ia * 2);
  int2 b = *reinterpret_cast<const int2*>(sxy + ib * 2);
  int2 c = *reinterpret_cast<const int2*>(sxy + ic * 2);
  if (a.x == RD_DROPPED || b.x == RD_DROPPED || c.x == RD_DROPPED) return 1;
  t.za = depth[ia];
  t.zb = depth[ib];
  t.zc = depth[ic];
  int64_t area2 = rd_edge(a.x, a.y, b.x, b.y, c.x, c.y);
  if (area2 == 0) return 2;
  if (area2 < 0) {                  // both windings are drawn: swap b and c
    const int2 q = b; b = c; c = q;
    const double z = t.zb; t.zb = t.zc; t.zc = z;
    area2 = -area2;
  }
  t.ax = a.x; t.ay = a.y; t.bx = b.x; t.by = b.y; t.cx = c.x; t.cy = c.y;
  t.area2 = area2;
  const int64_t xmin = min((int64_t)a.x, min((int64_t)b.x, (int64_t)c.x)), xmax = max((int64_t)a.x, max((int64_t)b.x, (int64_t)c.x));
  const int64_t ymin = min((int64_t)a.y, min((int64_t)b.y, (int64_t)c.y)), ymax = max((int64_t)a.y, max((int64_t)b.y, (int64_t)c.y));
  // pixel i has its samples at 256 i + [omin, omax]: the first pixel whose last sample >= min, the last whose first
  // sample <= max (one sample: the first centre >= min, the last <= max)
  constexpr int omin = rd_sample_min(S), omax = rd_sample_max(S);
  t.x0 = max(rd_floor_div256(xmin - omax + RD_SUB - 1), 0);
  t.y0 = max(rd_floor_div256(ymin - omax + RD_SUB - 1), 0);
  t.x1 = min(rd_floor_div256(xmax - omin), size - 1);
  t.y1 = min(rd_floor_div256(ymax - omin), size - 1);
  return 0;
}

// px: the S keys of pixel (x, y).  The edge functions are affine: evaluated once, at sample 0, and stepped to the other
// samples by exact int64 increments.
template <int S>
__device__ __forceinline__ void rd_pixel(const RdTri& t, int x, int y, uint32_t tri, uint64_t* __restrict__ px) {
  const int64_t qx = (int64_t)x * RD_SUB + rd_sample(S, 0, 0), qy = (int64_t)y * RD_SUB + rd_sample(S, 0, 1);
  const int64_t ea0 = rd_edge(t.bx, t.by, t.cx, t.cy, qx, qy);   // weight of a
  const int64_t eb0 = rd_edge(t.cx, t.cy, t.ax, t.ay, qx, qy);   // weight of b
  const int64_t ec0 = rd_edge(t.ax, t.ay, t.bx, t.by, qx, qy);   // weight of c
  const bool oa = rd_owns(t.bx, t.by, t.cx, t.cy), ob = rd_owns(t.cx, t.cy, t.ax, t.ay),
             oc = rd_owns(t.ax, t.ay, t.bx, t.by);
  constexpr int unroll = S > 4 ? 4 : S;   // 16 samples unrolled whole hold 244 VGPRs, by fours 80
#pragma unroll unroll
  for (int s = 0; s < S; ++s) {
    const int64_t dx = rd_sample(S, s, 0) - rd_sample(S, 0, 0), dy = rd_sample(S, s, 1) - rd_sample(S, 0, 1);
    const int64_t ea = ea0 + ((t.cx - t.bx) * dy - (t.cy - t.by) * dx);
    const int64_t eb = eb0 + ((t.ax - t.cx) * dy - (t.ay - t.cy) * dx);
    const int64_t ec = ec0 + ((t.bx - t.ax) * dy - (t.by - t.ay) * dx);
    const bool in = (ea > 0 || (ea == 0 && oa)) && (eb > 0 || (eb == 0 && ob)) && (ec > 0 || (ec == 0 && oc));
    if (!in) continue;
    // individually rounded, in this order.  Plain operators under this unit's `fp contract(off)`: the __dmul_rn /
    // __dadd_rn intrinsics are inline functions compiled under the header's default contraction, and hipcc fuses
    // them into v_fmac_f64 once they are inlined here.
    const double z = ((double)ea * t.za + (double)eb * t.zb) + (double)ec * t.zc;
    const double d = z / (double)t.area2;
    double q = d * 4294967296.0;
    if (!(q >= 0.0)) q = 0.0;
    if (q > 4294967295.0) q = 4294967295.0;
    const uint64_t key = ((uint64_t)(uint32_t)q << 32) | tri;
    if (key < px[s]) atomicMin((unsigned long long*)(px + s), (unsigned long long)key);   // keys only ever decrease
  }
}

// small path: grid (face blocks, mesh, view)
template <int S>
__global__ __launch_bounds__(RD_T) void rd_small_kernel(const int32_t* __restrict__ faces,
                                                        const int64_t* __restrict__ offs, int batch,
                                                        int64_t total_verts, int views, int size,
                                                        const int32_t* __restrict__ sxy,
                                                        const double* __restrict__ depth, int64_t big_px,
                                                        uint64_t* __restrict__ keys, int32_t* __restrict__ dropped,
                                                        unsigned long long* __restrict__ big_count,
                                                        uint64_t* __restrict__ big_list) {
  const int b = blockIdx.y, view = blockIdx.z;
  const int64_t f = (int64_t)blockIdx.x * RD_T + threadIdx.x;
  const int64_t nf = offs[3 * batch + b];
  const int lane = threadIdx.x & 63;
  int state = 3;                    // 3: no triangle
  RdTri t;
  if (f < nf) {
    const int32_t* F = faces + (offs[2 * batch + b] + f) * 3;
    const int64_t base = (int64_t)view * total_verts + offs[b];
    state = rd_setup<S>(sxy, depth, base + F[0], base + F[1], base + F[2], size, t);
  }
  const uint64_t drop = __ballot(state == 1);
  if (drop && lane == 0) atomicAdd(dropped + b * views + view, (int)__popcll(drop));
  const bool live = state == 0 && t.x0 <= t.x1 && t.y0 <= t.y1;
  const int64_t npx = live ? (int64_t)(t.x1 - t.x0 + 1) * (t.y1 - t.y0 + 1) : 0;
  const bool big = npx > big_px;
  const uint64_t bm = __ballot(big);
  if (bm) {                         // one counter bump per wave; the list's order does not matter
    unsigned long long at = 0;
    if (lane == __ffsll((unsigned long long)bm) - 1) at = atomicAdd(big_count, (unsigned long long)__popcll(bm));
    at = __shfl(at, __ffsll((unsigned long long)bm) - 1);
    if (big) big_list[at + __popcll(bm & ((1ull << lane) - 1))] = ((uint64_t)(b * views + view) << 32) | (uint32_t)f;
  }
  if (!live || big) return;
  uint64_t* img = keys + (int64_t)(b * views + view) * size * size * S;
  for (int y = t.y0; y <= t.y1; ++y)
    for (int x = t.x0; x <= t.x1; ++x) rd_pixel<S>(t, x, y, (uint32_t)f, img + ((int64_t)y * size + x) * S);
}

// large path: a wave per listed triangle, lanes over the pixels of its box
template <int S>
__global__ __launch_bounds__(RD_T) void rd_big_kernel(const int32_t* __restrict__ faces,
                                                      const int64_t* __restrict__ offs, int batch,
                                                      int64_t total_verts, int views, int size,
                                                      const int32_t* __restrict__ sxy,
                                                      const double* __restrict__ depth, uint64_t* __restrict__ keys,
                                                      const unsigned long long* __restrict__ big_count,
                                                      const uint64_t* __restrict__ big_list) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = (int64_t)gridDim.x * (RD_T / 64);
  const int64_t n = (int64_t)*big_count;
  for (int64_t k = (int64_t)blockIdx.x * (RD_T / 64) + (threadIdx.x >> 6); k < n; k += waves) {
    const uint64_t e = big_list[k];
    const int bv = (int)(e >> 32), b = bv / views, view = bv - b * views;
    const uint32_t f = (uint32_t)e;
    const int32_t* F = faces + (offs[2 * batch + b] + f) * 3;
    const int64_t base = (int64_t)view * total_verts + offs[b];
    RdTri t;
    if (rd_setup<S>(sxy, depth, base + F[0], base + F[1], base + F[2], size, t) != 0) continue;   // (cannot happen)
    const int w = t.x1 - t.x0 + 1;
    const int64_t npx = (int64_t)w * (t.y1 - t.y0 + 1);
    uint64_t* img = keys + (int64_t)bv * size * size * S;
    for (int64_t p = lane; p < npx; p += 64) {
      const int y = t.y0 + (int)(p / w), x = t.x0 + (int)(p % w);
      rd_pixel<S>(t, x, y, f, img + ((int64_t)y * size + x) * S);
    }
  }
}

// ---- shading -------------------------------------------------------------------------------------------------------
struct RdShade {
  double base[3], metallic, roughness, i_dir, i_point, i_spot, spot_scale, spot_offset, bg[3], tan_half;
};

struct RdV3 { double x, y, z; };
__device__ __forceinline__ RdV3 rd_sub(RdV3 a, RdV3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double rd_dot(RdV3 a, RdV3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ RdV3 rd_cross(RdV3 a, RdV3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ RdV3 rd_scale(RdV3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }

constexpr double RD_PI = 3.141592653589793;

// radiance * max(N.L, 0) * (diffuse + specular) of one light, added to out[3]
__device__ __forceinline__ void rd_light(const RdShade& S, RdV3 N, RdV3 V, RdV3 L, double radiance, double* out) {
  const double nl = rd_dot(N, L);
  if (!(nl > 0.0) || !(radiance > 0.0)) return;
  const RdV3 hs = {L.x + V.x, L.y + V.y, L.z + V.z};
  const double hh = rd_dot(hs, hs);
  if (!(hh > 0.0)) return;
  const RdV3 H = rd_scale(hs, 1.0 / sqrt(hh));
  const double nv = fabs(rd_dot(N, V)), nh = rd_dot(N, H);
  double x = 1.0 - rd_dot(V, H);
  if (!(x > 0.0)) x = 0.0;
  const double x2 = x * x, x5 = (x2 * x2) * x;
  const double al = S.roughness * S.roughness, a2 = al * al;
  const double dd = (nh * nh) * (a2 - 1.0) + 1.0;
  const double D = nh > 0.0 ? a2 / ((RD_PI * dd) * dd) : 0.0;
  const double vis = 1.0 / ((nl + sqrt(a2 + (1.0 - a2) * (nl * nl))) * (nv + sqrt(a2 + (1.0 - a2) * (nv * nv))));
  const double dv = D * vis, rn = radiance * nl;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double f0 = 0.04 * (1.0 - S.metallic) + S.base[c] * S.metallic;
    const double cd = S.base[c] * (1.0 - S.metallic);
    const double F = f0 + (1.0 - f0) * x5;
    out[c] += rn * ((1.0 - F) * (cd / RD_PI) + F * dv);
  }
}

// the unclamped colour of one face of mesh b at the ray through the centre of pixel (x, y), which need not hit it
__device__ __forceinline__ void rd_face_colour(const RdShade& S, const float* __restrict__ V0,
                                               const int32_t* __restrict__ F, const double* __restrict__ nrm,
                                               const double* __restrict__ M, int x, int y, int size, double* col) {
  const double s = nrm[3];
  const RdV3 ctr = {nrm[0], nrm[1], nrm[2]};
  RdV3 P3[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float* q = V0 + (int64_t)F[k] * 3;
    P3[k] = {((double)q[0] - ctr.x) / s, ((double)q[1] - ctr.y) / s, ((double)q[2] - ctr.z) / s};
  }
  const RdV3 eye = {M[3], M[7], M[11]}, zax = {M[2], M[6], M[10]};
  const double u = (((double)x + 0.5) / (double)size * 2.0 - 1.0) * S.tan_half;
  const double v = (1.0 - ((double)y + 0.5) / (double)size * 2.0) * S.tan_half;
  const RdV3 dir = {(M[0] * u + M[1] * v) - M[2], (M[4] * u + M[5] * v) - M[6], (M[8] * u + M[9] * v) - M[10]};
  const RdV3 n = rd_cross(rd_sub(P3[1], P3[0]), rd_sub(P3[2], P3[0]));
  const double den = rd_dot(n, dir);
  RdV3 pos;
  if (den != 0.0) {
    const double t = rd_dot(n, rd_sub(P3[0], eye)) / den;
    pos = {eye.x + t * dir.x, eye.y + t * dir.y, eye.z + t * dir.z};
  } else {
    pos = {((P3[0].x + P3[1].x) + P3[2].x) / 3.0, ((P3[0].y + P3[1].y) + P3[2].y) / 3.0,
           ((P3[0].z + P3[1].z) + P3[2].z) / 3.0};
  }
  const RdV3 lv = rd_sub(eye, pos);
  double d2 = rd_dot(lv, lv);
  if (!(d2 >= 1e-12)) d2 = 1e-12;
  const RdV3 V = rd_scale(lv, 1.0 / sqrt(d2));
  const double nn = rd_dot(n, n);
  RdV3 N = nn > 0.0 ? rd_scale(n, 1.0 / sqrt(nn)) : V;
  if (rd_dot(N, V) < 0.0) N = {-N.x, -N.y, -N.z};
  col[0] = col[1] = col[2] = 0.0;
  rd_light(S, N, V, zax, S.i_dir, col);                       // directional: along the camera's -z
  rd_light(S, N, V, V, S.i_point / d2, col);                  // point light at the eye
  double sa = rd_dot(zax, V) * S.spot_scale + S.spot_offset;  // spot: axis -z, cone between inner and outer
  sa = sa > 0.0 ? (sa < 1.0 ? sa : 1.0) : 0.0;
  rd_light(S, N, V, V, (S.i_spot / d2) * (sa * sa), col);
}

// a NaN becomes 0
__device__ __forceinline__ double rd_clamp01(double q) { return q > 0.0 ? (q < 1.0 ? q : 1.0) : 0.0; }

// one thread per pixel: every distinct face among the pixel's NS samples is shaded once, each sample takes the clamped
// colour of its face (or the background), and the mean, summed in sample order, is quantised once
template <int NS>
__global__ __launch_bounds__(RD_T) void rd_shade_kernel(const float* __restrict__ verts,
                                                        const int32_t* __restrict__ faces,
                                                        const int64_t* __restrict__ offs, int batch,
                                                        const double* __restrict__ norm,
                                                        const double* __restrict__ cam, int views, int size,
                                                        const uint64_t* __restrict__ keys, RdShade S,
                                                        uint8_t* __restrict__ image) {
  const int64_t npix = (int64_t)size * size;
  const int64_t p = (int64_t)blockIdx.x * RD_T + threadIdx.x;
  if (p >= npix) return;
  const int bv = blockIdx.y, b = bv / views, view = bv - b * views;
  const uint64_t* kp = keys + ((int64_t)bv * npix + p) * NS;
  uint8_t* o = image + ((int64_t)bv * npix + p) * 3;
  const int y = (int)(p / size), x = (int)(p - (int64_t)y * size);
  uint32_t id[NS];                  // the face of a sample; a face index is < 2^31, so all ones is the empty key
  double col[NS][3];
  uint32_t todo = 0;                // samples whose face is not shaded yet
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    id[s] = (uint32_t)kp[s];
    if (id[s] != 0xFFFFFFFFu) todo |= 1u << s;
#pragma unroll
    for (int c = 0; c < 3; ++c) col[s][c] = rd_clamp01(S.bg[c]);
  }
  while (todo) {                    // once per distinct face
    const int first = __ffs(todo) - 1;
    uint32_t face = id[0];
#pragma unroll
    for (int s = 1; s < NS; ++s) face = s == first ? id[s] : face;
    double fc[3];
    rd_face_colour(S, verts + offs[b] * 3, faces + (offs[2 * batch + b] + (int64_t)face) * 3, norm + b * 4,
                   cam + (int64_t)view * 24 + 12, x, y, size, fc);
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (((todo >> s) & 1u) && id[s] == face) {
#pragma unroll
        for (int c = 0; c < 3; ++c) col[s][c] = rd_clamp01(fc[c]);
        todo &= ~(1u << s);
      }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double q = col[0][c];
#pragma unroll
    for (int s = 1; s < NS; ++s) q = q + col[s][c];
    q = q / (double)NS;
    o[c] = (uint8_t)floor(255.0 * q + 0.5);
  }
}

bool rd_args_ok(int batch, int64_t total_verts, int views, int size) {
  return batch >= 1 && batch <= 65535 && views >= 1 && views <= 65535 && (int64_t)batch * views <= 65535 &&
         size >= 1 && size <= OFX_RENDER_MAX_SIZE && total_verts >= 1 && total_verts <= INT32_MAX;
}

}  // namespace

extern "C" int ofx_render_project(const float* verts, const int64_t* offs, int batch, int64_t total_verts,
                                  int64_t max_verts, const double* cam, int views, int size, double tan_half_fov,
                                  double znear, double zfar, int normalize, double* norm, int32_t* sxy, double* depth,
                                  void* stream) {
  if (!verts || !offs || !cam || !norm || !sxy || !depth || !rd_args_ok(batch, total_verts, views, size) ||
      max_verts < 1 || max_verts > total_verts || !(tan_half_fov > 0.0) || !(znear > 0.0) || !(zfar > znear))
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  rd_norm_kernel<<<batch, RD_NORM_T, 0, st>>>(verts, offs, batch, normalize ? 1 : 0, norm);
  OFX_LAUNCH_CHECK();
  // window depth (z_ndc + 1) / 2 = dep_a - dep_b / w
  const double dep_a = ((zfar + znear) / (zfar - znear) + 1.0) * 0.5, dep_b = (zfar * znear) / (zfar - znear);
  const dim3 grid((unsigned)ofx_cdiv(max_verts, RD_T), (unsigned)batch, (unsigned)views);
  rd_project_kernel<<<grid, RD_T, 0, st>>>(verts, offs, batch, total_verts, cam, norm, 1.0 / tan_half_fov,
                                           (double)size * (RD_SUB / 2), znear, dep_a, dep_b, sxy, depth);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" size_t ofx_render_raster_ws_bytes(int views, int64_t total_faces) {
  if (views < 1 || total_faces < 1) return 0;
  return 256 + (size_t)views * (size_t)total_faces * sizeof(uint64_t);
}

namespace {

template <int S>
int rd_raster(const int32_t* faces, const int64_t* offs, int batch, int64_t total_verts, int64_t max_faces, int views,
              int size, const int32_t* sxy, const double* depth, int64_t big_px, uint64_t* keys, int32_t* dropped,
              void* ws, hipStream_t st) {
  unsigned long long* big_count = (unsigned long long*)ws;
  uint64_t* big_list = (uint64_t*)((char*)ws + 256);
  if (hipMemsetAsync(keys, 0xFF, (size_t)batch * views * size * size * S * sizeof(uint64_t), st) != hipSuccess ||
      hipMemsetAsync(dropped, 0, (size_t)batch * views * sizeof(int32_t), st) != hipSuccess ||
      hipMemsetAsync(big_count, 0, sizeof(unsigned long long), st) != hipSuccess)
    return OFX_ELAUNCH;
  const dim3 grid((unsigned)ofx_cdiv(max_faces, RD_T), (unsigned)batch, (unsigned)views);
  rd_small_kernel<S><<<grid, RD_T, 0, st>>>(faces, offs, batch, total_verts, views, size, sxy, depth, big_px, keys,
                                            dropped, big_count, big_list);
  OFX_LAUNCH_CHECK();
  rd_big_kernel<S><<<RD_BIG_BLOCKS, RD_T, 0, st>>>(faces, offs, batch, total_verts, views, size, sxy, depth, keys,
                                                   big_count, big_list);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

template <int NS>
int rd_shade(const float* verts, const int32_t* faces, const int64_t* offs, int batch, const double* norm,
             const double* cam, int views, int size, const uint64_t* keys, const RdShade& S, uint8_t* image,
             hipStream_t st) {
  const dim3 grid((unsigned)ofx_cdiv((int64_t)size * size, RD_T), (unsigned)(batch * views));
  rd_shade_kernel<NS><<<grid, RD_T, 0, st>>>(verts, faces, offs, batch, norm, cam, views, size, keys, S, image);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

bool rd_samples_ok(int samples) { return samples == 1 || samples == 4 || samples == 16; }

}  // namespace

extern "C" int ofx_render_sample_offsets(int samples, int32_t* xy) {
  if (!xy || !rd_samples_ok(samples)) return OFX_EINVAL;
  for (int s = 0; s < samples; ++s) {
    xy[s * 2] = rd_sample(samples, s, 0);
    xy[s * 2 + 1] = rd_sample(samples, s, 1);
  }
  return OFX_OK;
}

extern "C" int ofx_render_raster_ms(const int32_t* faces, const int64_t* offs, int batch, int64_t total_verts,
                                    int64_t total_faces, int64_t max_faces, int views, int size, int samples,
                                    const int32_t* sxy, const double* depth, int64_t big_px, uint64_t* keys,
                                    int32_t* dropped, void* ws, void* stream) {
  if (!faces || !offs || !sxy || !depth || !keys || !dropped || !ws || !rd_args_ok(batch, total_verts, views, size) ||
      total_faces < 1 || total_faces > INT32_MAX || max_faces < 1 || max_faces > total_faces || big_px < 0 ||
      !rd_samples_ok(samples))
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  auto raster = samples == 4 ? rd_raster<4> : samples == 16 ? rd_raster<16> : rd_raster<1>;
  return raster(faces, offs, batch, total_verts, max_faces, views, size, sxy, depth, big_px, keys, dropped, ws, st);
}

extern "C" int ofx_render_raster(const int32_t* faces, const int64_t* offs, int batch, int64_t total_verts,
                                 int64_t total_faces, int64_t max_faces, int views, int size, const int32_t* sxy,
                                 const double* depth, int64_t big_px, uint64_t* keys, int32_t* dropped, void* ws,
                                 void* stream) {
  return ofx_render_raster_ms(faces, offs, batch, total_verts, total_faces, max_faces, views, size, 1, sxy, depth,
                              big_px, keys, dropped, ws, stream);
}

extern "C" int ofx_render_shade_ms(const float* verts, const int32_t* faces, const int64_t* offs, int batch,
                                   const double* norm, const double* cam, int views, int size, int samples,
                                   double tan_half_fov, const uint64_t* keys, const double* params, uint8_t* image,
                                   void* stream) {
  if (!verts || !faces || !offs || !norm || !cam || !keys || !params || !image || batch < 1 || views < 1 ||
      (int64_t)batch * views > 65535 || size < 1 || size > OFX_RENDER_MAX_SIZE || !(tan_half_fov > 0.0) ||
      !rd_samples_ok(samples))
    return OFX_EINVAL;
  RdShade S;
  for (int c = 0; c < 3; ++c) S.base[c] = params[c];
  S.metallic = params[3];
  S.roughness = params[4];
  S.i_dir = params[5];
  S.i_point = params[6];
  S.i_spot = params[7];
  S.spot_scale = params[8];
  S.spot_offset = params[9];
  for (int c = 0; c < 3; ++c) S.bg[c] = params[10 + c];
  S.tan_half = tan_half_fov;
  hipStream_t st = ofx_stream(stream);
  auto shade = samples == 4 ? rd_shade<4> : samples == 16 ? rd_shade<16> : rd_shade<1>;
  return shade(verts, faces, offs, batch, norm, cam, views, size, keys, S, image, st);
}

extern "C" int ofx_render_shade(const float* verts, const int32_t* faces, const int64_t* offs, int batch,
                                const double* norm, const double* cam, int views, int size, double tan_half_fov,
                                const uint64_t* keys, const double* params, uint8_t* image, void* stream) {
  return ofx_render_shade_ms(verts, faces, offs, batch, norm, cam, views, size, 1, tan_half_fov, keys, params, image,
                             stream);
}

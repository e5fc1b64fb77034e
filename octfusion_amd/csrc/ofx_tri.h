// Point-triangle arithmetic shared by the lattice entry (ofx_mesh2sdf.hip) and the query entry (ofx_meshquery.hip):
// the culling bounds with their margins, the fp64 point-triangle pair on a staged record, and the ray-parity crossing
// with its exact edge functions.  One copy, so that both entries minimise the SAME expression and count the SAME
// crossings, bit for bit.  Include it after `#pragma clang fp contract(off)`: every operation here is rounded on its
// own.  DESIGN.md sections 4.11 and 4.19.
#pragma once
#include "ofx_common.h"

#include <cmath>

constexpr int MS_T = 64;           // one wave per block
constexpr int MS_REC = 16;         // doubles per staged triangle
constexpr float MS_REL = 1.0e-3f;  // margins of every skip: relative, and absolute in squared distance
constexpr float MS_ABS = 1.0e-4f;

// order-preserving int key of a float
__device__ __forceinline__ int32_t ms_key(float f) {
  const int32_t b = __float_as_int(f);
  return b >= 0 ? b : b ^ 0x7fffffff;
}
__device__ __forceinline__ float ms_unkey(int32_t k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

// Shape of global item t (off [batch + 1] is non-decreasing; batch is small): the last b with off[b] <= t.
__device__ __forceinline__ int ms_shape_of(const int64_t* __restrict__ off, int batch, int64_t t) {
  int lo = 0, hi = batch - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= t) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The nine coordinates of triangle t of shape b; false (nothing read past the shape) if an index is out of range or a
// coordinate is not finite.
__device__ __forceinline__ bool ms_load(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                        const int64_t* __restrict__ vert_off, int64_t t, int b, float (&c)[9]) {
  const int64_t v0 = vert_off[b], nv = vert_off[b + 1] - v0;
  bool ok = true;
  int32_t id[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    id[k] = faces[t * 3 + k];
    ok = ok && id[k] >= 0 && (int64_t)id[k] < nv;
  }
  if (!ok) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      c[k * 3 + a] = verts[(v0 + id[k]) * 3 + a];
      ok = ok && isfinite(c[k * 3 + a]);
    }
  return ok;
}

__device__ __forceinline__ float ms_wave_max(float v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = fmaxf(v, __shfl_xor(v, s));
  return v;
}
__device__ __forceinline__ float ms_wave_min(float v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = fminf(v, __shfl_xor(v, s));
  return v;
}

// squared smallest / largest distance between the boxes [alo, ahi] and [blo, bhi]
__device__ __forceinline__ float ms_box_min2(const float (&alo)[3], const float (&ahi)[3], const float (&blo)[3],
                                             const float (&bhi)[3]) {
  float s = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float g = fmaxf(0.f, fmaxf(blo[a] - ahi[a], alo[a] - bhi[a]));
    s += g * g;
  }
  return s;
}
__device__ __forceinline__ float ms_box_max2(const float (&alo)[3], const float (&ahi)[3], const float (&blo)[3],
                                             const float (&bhi)[3]) {
  float s = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float g = fmaxf(fabsf(bhi[a] - alo[a]), fabsf(ahi[a] - blo[a]));
    s += g * g;
  }
  return s;
}
__device__ __forceinline__ bool ms_beyond(float lower, float upper) { return lower * (1.f - MS_REL) > upper + MS_ABS; }

__device__ __forceinline__ void ms_bin_box(const int32_t* __restrict__ box, int64_t bin, float (&lo)[3],
                                           float (&hi)[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = ms_unkey(box[bin * 6 + a]);
    hi[a] = ms_unkey(box[bin * 6 + 3 + a]);
  }
}

__device__ __forceinline__ double ms_dot(const double (&u)[3], const double (&v)[3]) {
  return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
}
__device__ __forceinline__ void ms_cross(const double (&u)[3], const double (&v)[3], double (&r)[3]) {
  r[0] = u[1] * v[2] - u[2] * v[1];
  r[1] = u[2] * v[0] - u[0] * v[2];
  r[2] = u[0] * v[1] - u[1] * v[0];
}
__device__ __forceinline__ double ms_inv(double x) { return x > 0.0 ? 1.0 / x : 0.0; }

// squared distance from the end of `ap` (= p - a) to the segment a + t e, t in [0, 1]; ie = 1 / |e|^2 or 0
__device__ __forceinline__ double ms_seg2(const double (&ap)[3], const double (&e)[3], double ie) {
  double t = ms_dot(ap, e) * ie;
  t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
  double d[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) d[a] = ap[a] - t * e[a];
  return ms_dot(d, d);
}

// ---- the pair -----------------------------------------------------------------------------------------------------
// Search one bin's triangles [start, start + count) for a wave whose points lie in the box [klo, khi]: lane's point p,
// running best (squared).  64 triangles at a time: each lane stages one triangle into rec [MS_REC][MS_T] (a, b - a,
// c - b, the normal, the reciprocals of the squared edge lengths and of |n|^2, 0 where the length is 0) unless its box
// is beyond the wave's worst best; the survivors are evaluated by all lanes.  FACE: a record is ten words, the tenth the
// face's index, staged in ids [MS_T]; face = the lowest index among the triangles whose squared distance equals best.
template <bool COUNT, bool FACE>
__device__ __forceinline__ void ms_search_bin(const float* __restrict__ tri, int64_t start, int count, int lane,
                                              const float (&klo)[3], const float (&khi)[3], const double (&p)[3],
                                              double& best, int32_t& face, double* rec, int32_t* ids,
                                              uint32_t (&tally)[3]) {
  constexpr int W = FACE ? 10 : 9;
  if (COUNT) {
    tally[0] += 1u;
    tally[1] += (uint32_t)count;
  }
  for (int base = 0; base < count; base += MS_T) {
    const int t = base + lane;
    bool keep = t < count;
    const float worst = ms_wave_max((float)best);
    if (keep) {
      float c[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) c[k] = tri[(start + t) * W + k];
      float lo[3], hi[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = fminf(fminf(c[a], c[3 + a]), c[6 + a]);
        hi[a] = fmaxf(fmaxf(c[a], c[3 + a]), c[6 + a]);
      }
      keep = !ms_beyond(ms_box_min2(klo, khi, lo, hi), worst);
      if (keep) {
        double A[3], ab[3], bc[3], ca[3], n[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          A[a] = (double)c[a];
          ab[a] = (double)c[3 + a] - (double)c[a];
          bc[a] = (double)c[6 + a] - (double)c[3 + a];
          ca[a] = (double)c[a] - (double)c[6 + a];
        }
        ms_cross(ab, bc, n);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          rec[a * MS_T + lane] = A[a];
          rec[(3 + a) * MS_T + lane] = ab[a];
          rec[(6 + a) * MS_T + lane] = bc[a];
          rec[(9 + a) * MS_T + lane] = n[a];
        }
        rec[12 * MS_T + lane] = ms_inv(ms_dot(ab, ab));
        rec[13 * MS_T + lane] = ms_inv(ms_dot(bc, bc));
        rec[14 * MS_T + lane] = ms_inv(ms_dot(ca, ca));
        rec[15 * MS_T + lane] = ms_inv(ms_dot(n, n));
        if constexpr (FACE) ids[lane] = __float_as_int(tri[(start + t) * W + 9]);
      }
    }
    __syncthreads();
    uint64_t mask = __ballot(keep);
    if (COUNT) tally[2] += (uint32_t)__popcll(mask);
    while (mask) {
      const int j = __ffsll((unsigned long long)mask) - 1;
      mask &= mask - 1;
      double ab[3], bc[3], ca[3], n[3], ap[3], bp[3], cp[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        ab[a] = rec[(3 + a) * MS_T + j];
        bc[a] = rec[(6 + a) * MS_T + j];
        n[a] = rec[(9 + a) * MS_T + j];
        ca[a] = -(ab[a] + bc[a]);          // only a direction for the clamp and the inside test of edge c -> a
        ap[a] = p[a] - rec[a * MS_T + j];
        bp[a] = ap[a] - ab[a];
        cp[a] = bp[a] - bc[a];
      }
      double d = ms_seg2(ap, ab, rec[12 * MS_T + j]);
      d = fmin(d, ms_seg2(bp, bc, rec[13 * MS_T + j]));
      d = fmin(d, ms_seg2(cp, ca, rec[14 * MS_T + j]));
      const double inn = rec[15 * MS_T + j];
      if (inn > 0.0) {
        double x[3];
        ms_cross(ab, ap, x);
        const double s0 = ms_dot(n, x);
        ms_cross(bc, bp, x);
        const double s1 = ms_dot(n, x);
        ms_cross(ca, cp, x);
        const double s2 = ms_dot(n, x);
        if (s0 >= 0.0 && s1 >= 0.0 && s2 >= 0.0) {
          const double h = ms_dot(n, ap);
          d = fmin(d, (h * h) * inn);
        }
      }
      if constexpr (FACE) {
        const int32_t id = ids[j];
        if (d < best || (d == best && id < face)) {
          best = d;
          face = id;
        }
      } else {
        best = fmin(best, d);
      }
    }
    __syncthreads();
  }
}

// The point of triangle c (nine coordinates) nearest to p: the branches of the pair above with the foot carried
// along -- the three edges as clamped segments (first a-b, then b-c, then c-a: a later one only if strictly nearer),
// then the plane where the projection falls inside and is strictly nearer.
__device__ __forceinline__ void ms_closest(const float (&c)[9], const double (&p)[3], double (&cl)[3]) {
  double ab[3], bc[3], ca[3], n[3], ap[3], bp[3], cp[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ab[a] = (double)c[3 + a] - (double)c[a];
    bc[a] = (double)c[6 + a] - (double)c[3 + a];
    ca[a] = (double)c[a] - (double)c[6 + a];
    ap[a] = p[a] - (double)c[a];
    bp[a] = p[a] - (double)c[3 + a];
    cp[a] = p[a] - (double)c[6 + a];
  }
  ms_cross(ab, bc, n);
  const double ie[3] = {ms_inv(ms_dot(ab, ab)), ms_inv(ms_dot(bc, bc)), ms_inv(ms_dot(ca, ca))};
  double best = INFINITY;
  auto edge = [&](const double (&vp)[3], const double (&e)[3], double inv) {
    const double d = ms_seg2(vp, e, inv);
    if (d < best) {
      best = d;
      double t = ms_dot(vp, e) * inv;
      t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
#pragma unroll
      for (int a = 0; a < 3; ++a) cl[a] = p[a] - (vp[a] - t * e[a]);
    }
  };
  edge(ap, ab, ie[0]);
  edge(bp, bc, ie[1]);
  edge(cp, ca, ie[2]);
  const double inn = ms_inv(ms_dot(n, n));
  if (inn > 0.0) {
    double x[3];
    ms_cross(ab, ap, x);
    const double s0 = ms_dot(n, x);
    ms_cross(bc, bp, x);
    const double s1 = ms_dot(n, x);
    ms_cross(ca, cp, x);
    const double s2 = ms_dot(n, x);
    const double h = ms_dot(n, ap);
    if (s0 >= 0.0 && s1 >= 0.0 && s2 >= 0.0 && (h * h) * inn < best) {
      const double k = h * inn;
#pragma unroll
      for (int a = 0; a < 3; ++a) cl[a] = p[a] - k * n[a];
    }
  }
}

// ---- sign ---------------------------------------------------------------------------------------------------------
// a*b - c*d with one rounding of the result (Kahan); exact whenever the products are
__device__ __forceinline__ double ms_det2(double a, double b, double c, double d) {
  const double w = c * d;
  const double e = fma(-c, d, w);
  const double f = fma(a, b, -w);
  return f + e;
}

// Edge function of the directed edge u -> v at q, (v - u) x (q - u) in the yz-plane, on the canonical ordering of the
// end points; sgn = its sign at q + (eps, eps^2).  Reversing the edge negates both, bit for bit.
__device__ __forceinline__ double ms_edge(double uy, double uz, double vy, double vz, double qy, double qz, int& sgn) {
  const bool flip = vy < uy || (vy == uy && vz < uz);
  const double ay = flip ? vy : uy, az = flip ? vz : uz, by = flip ? uy : vy, bz = flip ? uz : vz;
  const double dy = by - ay, dz = bz - az;
  const double e = ms_det2(dy, qz - az, dz, qy - ay);
  int s = e > 0.0 ? 1 : (e < 0.0 ? -1 : 0);
  if (s == 0) s = dz != 0.0 ? (dz > 0.0 ? -1 : 1) : (dy > 0.0 ? 1 : -1);
  sgn = flip ? -s : s;
  return flip ? -e : e;
}

// Doubled signed area of the yz-projection (y0, z0), (y1, z1), (y2, z2); a projection of zero area never counts.
__device__ __forceinline__ double ms_proj_area(double y0, double z0, double y1, double z1, double y2, double z2) {
  return ms_det2(y1 - y0, z2 - z0, z1 - z0, y2 - y0);
}

// x of the crossing of the ray through a point of the yz-plane with the triangle staged in column q of rec (rows 0-5
// the projected corners y0 z0 y1 z1 y2 z2, 6 x of corner 0, 7 and 8 the x extents of edges 0-1 and 0-2, 9 the projected
// area), given e01 and e20, the edge functions of edges 0-1 and 2-0 at the point (the weights of corners 2 and 1).  The
// ray crosses iff the three ms_edge signs agree.
__device__ __forceinline__ double ms_cross_x(const double* rec, int q, double e01, double e20) {
  return rec[6 * MS_T + q] + (e01 * rec[8 * MS_T + q] + e20 * rec[7 * MS_T + q]) / rec[9 * MS_T + q];
}

// Generalized winding numbers of arbitrary points around triangle meshes: the robust inside / outside of open,
// self-intersecting or nested soups (Jacobson et al. 2013; the far field after Barill et al. 2018, first order).  The
// third client of the triangle bins (ofx_tribins.h).  Contract: include/ofx.h; tests/winding_oracle.py restates it in
// float64.  DESIGN.md section 4.21 has the order argument and the figures.
//
//   pair    van Oosterom and Strackee's solid angle of a triangle seen from the query, in fp64 with every operation
//           rounded on its own (wn_pair): one expression of (query, triangle).  A triangle whose fp64 (b - a) x (c - a)
//           is exactly zero is never staged.
//   exact   beta == 0.  One wave per 64 consecutive queries of one shape; the shape's faces are staged through LDS 64
//           at a time, in face-index order and straight from the caller's arrays, and every lane adds the staged pairs
//           in that order: the sum of a query is one fixed chain over the shape's faces, whatever its lane, wave or
//           batch.  Nothing here reads the bins, so they are not built (only the status words are) and the queries
//           are not sorted: every wave meets every face anyway.
//   far     beta > 0.  The bins are built; wn_rank_kernel puts every bin's face indices in rising order (the fill's
//           integer atomics hand out the slots of a bin in an order that changes from run to run); wn_moment_kernel
//           sums each bin's dipole moment N, area-weighted centre and radius over that order; one wave per 64
//           Morton-neighbouring queries (ofx_tribins_order_points) then visits the bins in bin-index order.  A lane
//           for which the bin is far adds the dipole; if any lane is near, the bin's faces are staged in face-index
//           order and the near lanes add their pairs, summed from zero per bin.  So the sum of a query is one fixed
//           chain over (bin, face), whatever the other lanes of its wave decide.
// No floating-point atomics anywhere.
#include "ofx_tribins.h"

#include <cmath>

#pragma clang fp contract(off)

#include "ofx_tri.h"

namespace {

constexpr int WN_MOM = 8;          // doubles per bin: N (3), centre (3), radius (-1: no triangle with an area), unused
constexpr double WN_4PI = 4.0 * 3.14159265358979323846;

// the meshes of a call and its queries
struct WnMesh : TbMesh {
  const float* q;
  const int64_t* q_off;
};

// (b - a) x (c - a) of the nine coordinates c, in fp64; true iff a component is not zero (the triangle counts)
__device__ __forceinline__ bool wn_normal(const float (&c)[9], double (&n)[3]) {
  double e1[3], e2[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    e1[a] = (double)c[3 + a] - (double)c[a];
    e2[a] = (double)c[6 + a] - (double)c[a];
  }
  ms_cross(e1, e2, n);
  return n[0] != 0.0 || n[1] != 0.0 || n[2] != 0.0;
}

// A face index read back from the ranked records is used only inside the shape (nothing is read through another).
__device__ __forceinline__ bool wn_face_ok(int32_t id, int64_t F) { return id >= 0 && (int64_t)id < F; }

// Lane's triangle (face t of the call, if `have`) into column `lane` of rec [9][MS_T]; whether it counts.
__device__ __forceinline__ bool wn_stage(const WnMesh& m, int b, int64_t t, bool have, int lane, double* rec) {
  float c[9];
  bool keep = have && ms_load(m.verts, m.faces, m.vert_off, t, b, c);
  if (keep) {
    double n[3];
    keep = wn_normal(c, n);
    if (keep) {
#pragma unroll
      for (int k = 0; k < 9; ++k) rec[k * MS_T + lane] = (double)c[k];
    }
  }
  return keep;
}

// ---- the pair -----------------------------------------------------------------------------------------------------
// atan2(num, den) of the triangle staged in column j seen from p: a, b, c = the vertices minus p,
// num = a . (b x c), den = |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|, summed from the left.
__device__ __forceinline__ double wn_pair(const double* rec, int j, const double (&p)[3]) {
  double a[3], b[3], c[3], x[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[k] = rec[k * MS_T + j] - p[k];
    b[k] = rec[(3 + k) * MS_T + j] - p[k];
    c[k] = rec[(6 + k) * MS_T + j] - p[k];
  }
  const double la = sqrt(ms_dot(a, a)), lb = sqrt(ms_dot(b, b)), lc = sqrt(ms_dot(c, c));
  ms_cross(b, c, x);
  const double num = ms_dot(a, x);
  const double den = (((la * lb) * lc + ms_dot(a, b) * lc) + ms_dot(b, c) * la) + ms_dot(c, a) * lb;
  return atan2(num, den);
}

// the winding number of a sum of atan2 terms: 2 S / 4 pi
__device__ __forceinline__ double wn_turns(double S) { return (2.0 * S) / WN_4PI; }

// the sum over the wave in one fixed butterfly: the same bits in every lane
__device__ __forceinline__ double wn_wave_sum(double v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
  return v;
}
__device__ __forceinline__ double wn_wave_max(double v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v = fmax(v, __shfl_xor(v, s));
  return v;
}

// ---- exact --------------------------------------------------------------------------------------------------------
template <bool COUNT>
__global__ __launch_bounds__(MS_T) void wn_exact_kernel(WnMesh m, const int32_t* __restrict__ status,
                                                        float* __restrict__ wind, unsigned long long* counters) {
  __shared__ double rec[9 * MS_T];
  const int b = blockIdx.y;
  if (status[b]) return;
  const int64_t q0 = m.q_off[b], nq = m.q_off[b + 1] - q0;
  if ((int64_t)blockIdx.x * MS_T >= nq) return;
  const int lane = threadIdx.x;
  const int64_t s = (int64_t)blockIdx.x * MS_T + lane;
  const int64_t qi = s < nq ? q0 + s : -1;
  bool fin = qi >= 0;
  double p[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float v = qi >= 0 ? m.q[qi * 3 + a] : 0.f;
    fin = fin && isfinite(v);
    p[a] = (double)v;
  }
  const uint32_t lanes = COUNT ? (uint32_t)__popcll(__ballot(fin)) : 0u;
  uint32_t staged = 0u;
  unsigned long long pairs = 0ull;
  const int64_t t0 = m.tri_off[b], F = m.tri_off[b + 1] - t0;
  double S = 0.0;
  for (int64_t base = 0; base < F; base += MS_T) {
    const bool keep = wn_stage(m, b, t0 + base + lane, base + lane < F, lane, rec);
    __syncthreads();
    uint64_t mask = __ballot(keep);
    if (COUNT) {
      staged += (uint32_t)__popcll(mask);
      pairs += (unsigned long long)__popcll(mask) * lanes;
    }
    while (mask) {
      const int j = __ffsll((unsigned long long)mask) - 1;
      mask &= mask - 1;
      S += wn_pair(rec, j, p);
    }
    __syncthreads();
  }
  if (qi >= 0) wind[qi] = fin ? (float)wn_turns(S) : NAN;
  if (COUNT && lane == 0) {
    atomicAdd(&counters[1], (unsigned long long)staged);
    atomicAdd(&counters[2], pairs);
  }
}

// ---- far field: the bins in face order, their moments -------------------------------------------------------------
// Word 9 of every record is its face; word 0 of slot off[bin] + (the number of lower faces in the bin) receives it:
// afterwards word 0 of a bin's slots lists the bin's faces in rising order.  Only word 9 is read and only word 0 is
// written here, each slot's word 0 by exactly one thread (a face is in one bin once), so the order of the threads does
// not matter.  The nine coordinates of the records are not used by this entry: it stages from the caller's arrays.
__global__ __launch_bounds__(TB_PREP_T) void wn_rank_kernel(TbBins w, int64_t nb) {
  const int64_t total = w.off[nb];
  const int64_t stride = (int64_t)gridDim.x * TB_PREP_T;
  for (int64_t s = (int64_t)blockIdx.x * TB_PREP_T + threadIdx.x; s < total; s += stride) {
    int64_t lo = 0, hi = nb - 1;                  // the last bin with off[bin] <= s: the one that holds slot s
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if ((int64_t)w.off[mid] <= s) lo = mid; else hi = mid - 1;
    }
    const int64_t start = w.off[lo], end = w.off[lo + 1];
    const int32_t id = __float_as_int(w.tri[s * TB_W + 9]);
    int64_t rank = 0;
    for (int64_t j = start; j < end; ++j) rank += __float_as_int(w.tri[j * TB_W + 9]) < id ? 1 : 0;
    w.tri[(start + rank) * TB_W] = __int_as_float(id);
  }
}

// One wave per bin: N = sum of (b - a) x (c - a) / 2, the centre = sum of area x centroid / sum of area, over the
// bin's triangles with an area in face order, 64 at a time (the wave's butterfly, then the running sum); then the
// radius = the largest distance from the centre to a vertex of those triangles.
__global__ __launch_bounds__(MS_T) void wn_moment_kernel(WnMesh m, TbBins w, const int32_t* __restrict__ status,
                                                         double* __restrict__ mom) {
  const int b = blockIdx.y, g = blockIdx.x;
  if (status[b]) return;
  const int G = tb_G(m, b);
  if (g >= G * G * G) return;
  const int64_t bin = (int64_t)b * m.GS + g;
  const int64_t start = w.off[bin];
  const int n = w.off[bin + 1] - (int32_t)start;
  if (n <= 0) return;                             // an empty bin is never looked up
  const int lane = threadIdx.x;
  const int64_t t0 = m.tri_off[b], F = m.tri_off[b + 1] - t0;
  double sum[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int base = 0; base < n; base += MS_T) {
    const bool have = base + lane < n;
    const int32_t id = have ? __float_as_int(w.tri[(start + base + lane) * TB_W]) : -1;
    float c[9];
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, nn[3];
    if (wn_face_ok(id, F) && ms_load(m.verts, m.faces, m.vert_off, t0 + id, b, c) && wn_normal(c, nn)) {
      const double area = 0.5 * sqrt(ms_dot(nn, nn));
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        v[a] = 0.5 * nn[a];
        v[3 + a] = area * ((((double)c[a] + (double)c[3 + a]) + (double)c[6 + a]) / 3.0);
      }
      v[6] = area;
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) sum[k] += wn_wave_sum(v[k]);
  }
  if (!(sum[6] > 0.0)) {                          // nothing with an area: the bin contributes nothing
    if (lane == 0) mom[bin * WN_MOM + 6] = -1.0;
    return;
  }
  double centre[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) centre[a] = sum[3 + a] / sum[6];
  double r2 = 0.0;
  for (int base = 0; base < n; base += MS_T) {
    const bool have = base + lane < n;
    const int32_t id = have ? __float_as_int(w.tri[(start + base + lane) * TB_W]) : -1;
    float c[9];
    double nn[3];
    if (wn_face_ok(id, F) && ms_load(m.verts, m.faces, m.vert_off, t0 + id, b, c) && wn_normal(c, nn)) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        double d[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = (double)c[k * 3 + a] - centre[a];
        r2 = fmax(r2, ms_dot(d, d));
      }
    }
  }
  r2 = wn_wave_max(r2);
  if (lane < 3) {
    mom[bin * WN_MOM + lane] = sum[lane];
    mom[bin * WN_MOM + 3 + lane] = centre[lane];
  }
  if (lane == 0) mom[bin * WN_MOM + 6] = sqrt(r2);
}

template <bool COUNT>
__global__ __launch_bounds__(MS_T) void wn_far_kernel(WnMesh m, TbBins w, TbOrder o, const double* __restrict__ mom,
                                                      const int32_t* __restrict__ status, double beta,
                                                      float* __restrict__ wind, unsigned long long* counters) {
  __shared__ double rec[9 * MS_T];
  const int b = blockIdx.y;
  if (status[b]) return;
  const int64_t q0 = m.q_off[b], nq = m.q_off[b + 1] - q0;
  if ((int64_t)blockIdx.x * MS_T >= nq) return;
  const int lane = threadIdx.x;
  const int64_t s = (int64_t)blockIdx.x * MS_T + lane;
  const int64_t qi = s < nq ? (int64_t)o.sidx[q0 + s] : -1;
  bool fin = qi >= 0;
  double p[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float v = qi >= 0 ? m.q[qi * 3 + a] : 0.f;
    fin = fin && isfinite(v);
    p[a] = (double)v;
  }
  uint32_t far_bins = 0u, staged = 0u;
  unsigned long long pairs = 0ull, dipoles = 0ull;
  const int G = tb_G(m, b), G3 = G * G * G;
  const int64_t bin0 = (int64_t)b * m.GS, t0 = m.tri_off[b], F = m.tri_off[b + 1] - t0;
  double acc = 0.0;
  for (int g = 0; g < G3; ++g) {
    const int64_t start = w.off[bin0 + g];
    const int n = w.off[bin0 + g + 1] - (int32_t)start;
    if (n <= 0) continue;
    const double* mk = mom + (bin0 + g) * WN_MOM;
    const double r = mk[6];
    if (r < 0.0) continue;                        // no triangle with an area
    double d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = mk[3 + a] - p[a];
    const double dist = sqrt(ms_dot(d, d));
    const bool far = dist > beta * r;
    const uint64_t near = __ballot(fin && !far);
    if (fin && far) {
      const double N[3] = {mk[0], mk[1], mk[2]};
      acc += ms_dot(N, d) / (WN_4PI * ((dist * dist) * dist));
    }
    if (COUNT) {
      dipoles += (unsigned long long)__popcll(__ballot(fin && far));
      far_bins += near == 0ull ? 1u : 0u;
    }
    if (near == 0ull) continue;
    double S = 0.0;
    for (int base = 0; base < n; base += MS_T) {
      const bool have = base + lane < n;
      const int32_t id = have ? __float_as_int(w.tri[(start + base + lane) * TB_W]) : -1;
      const bool keep = wn_stage(m, b, t0 + id, wn_face_ok(id, F), lane, rec);
      __syncthreads();
      uint64_t mask = __ballot(keep);
      if (COUNT) {
        staged += (uint32_t)__popcll(mask);
        pairs += (unsigned long long)__popcll(mask) * (unsigned long long)__popcll(near);
      }
      while (mask) {
        const int j = __ffsll((unsigned long long)mask) - 1;
        mask &= mask - 1;
        S += wn_pair(rec, j, p);
      }
      __syncthreads();
    }
    if (fin && !far) acc += wn_turns(S);
  }
  if (qi >= 0) wind[qi] = fin ? (float)acc : NAN;
  if (COUNT && lane == 0) {
    atomicAdd(&counters[0], (unsigned long long)far_bins);
    atomicAdd(&counters[1], (unsigned long long)staged);
    atomicAdd(&counters[2], pairs);
    atomicAdd(&counters[3], dipoles);
  }
}

unsigned long long* wn_counters = nullptr;      // ofx_mesh_winding_set_counters

size_t wn_mom_bytes(int batch, int bins) {
  return tb_align((size_t)batch * tb_stride(bins) * WN_MOM * sizeof(double));
}

}  // namespace

extern "C" size_t ofx_mesh_winding_ws_bytes(int batch, int64_t total_verts, int64_t total_faces, int64_t total_q,
                                            int bins) {
  if (!ofx_tribins_args_ok(batch, total_verts, total_faces, total_q, bins)) return 0;
  return wn_mom_bytes(batch, bins) + ofx_tribins_layout(batch, total_faces, total_q, bins, nullptr, nullptr, nullptr);
}

extern "C" int ofx_mesh_winding_set_counters(unsigned long long* words) {
  wn_counters = words;
  return OFX_OK;
}

extern "C" int ofx_mesh_winding(const float* verts, const int32_t* faces, const int64_t* vert_off,
                                const int64_t* tri_off, const float* q, const int64_t* q_off, int batch,
                                int64_t total_q, int64_t max_q, int bins, float beta, float* wind, void* ws,
                                int32_t* status, void* stream) {
  if (!verts || !faces || !vert_off || !tri_off || !q_off || !ws || !status ||
      !ofx_tribins_args_ok(batch, 1, 1, total_q, bins) || max_q < 0 || max_q > total_q ||
      (total_q > 0 && (!q || !wind || max_q < 1)) || !(beta >= 0.f) || !std::isfinite(beta))
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  double* mom = (double*)ws;                      // first, so that no offset depends on the face count
  TbBins w;
  TbOrder o;
  ofx_tribins_layout(batch, 0, total_q, bins, (char*)ws + wn_mom_bytes(batch, bins), &w, &o);
  const WnMesh m{{verts, faces, vert_off, tri_off, batch, bins, tb_stride(bins)}, q, q_off};
  const bool far = beta > 0.f;
  // exact mode reads no bin: the build stops after the status words and the shapes' boxes
  int rc = ofx_tribins_build(m, w, far ? total_q : 0, status, stream);
  if (rc || total_q == 0) return rc;              // no queries: the status words are still written
  const dim3 waves((unsigned)ofx_cdiv(max_q, MS_T), (unsigned)batch);
  if (!far) {
    if (wn_counters) wn_exact_kernel<true><<<waves, MS_T, 0, st>>>(m, status, wind, wn_counters);
    else wn_exact_kernel<false><<<waves, MS_T, 0, st>>>(m, status, wind, nullptr);
    OFX_LAUNCH_CHECK();
    return OFX_OK;
  }
  wn_rank_kernel<<<2048, TB_PREP_T, 0, st>>>(w, (int64_t)batch * m.GS);
  OFX_LAUNCH_CHECK();
  const int G = bins ? bins : TB_MAX_G;
  wn_moment_kernel<<<dim3((unsigned)(G * G * G), (unsigned)batch), MS_T, 0, st>>>(m, w, status, mom);
  OFX_LAUNCH_CHECK();
  rc = ofx_tribins_order_points(m, q, q_off, w, o, total_q, stream);
  if (rc) return rc;
  if (wn_counters) wn_far_kernel<true><<<waves, MS_T, 0, st>>>(m, w, o, mom, status, (double)beta, wind, wn_counters);
  else wn_far_kernel<false><<<waves, MS_T, 0, st>>>(m, w, o, mom, status, (double)beta, wind, nullptr);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

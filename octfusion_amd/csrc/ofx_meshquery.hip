// Exact point-to-mesh queries: distance, face and closest point of arbitrary points against triangle meshes, the
// search of ofx_mesh2sdf.hip lifted off the lattice.  Contract: include/ofx.h; tests/meshquery_oracle.py restates it in
// float64 (brute force, Ericson's regions).  DESIGN.md section 4.19 has the exactness argument and the figures.
//
//   bins   the per-shape G^3 centroid bins of ofx_tribins.h, built by ofx_tribins_build: the structure the ray casts
//          search too.  G is given or comes from the shape's face count (tb_bins).  Nothing below depends on which
//          bin a triangle is in or on the order inside a bin.
//   order  ofx_tribins_order_points: a key per query, shape << 32 | non-finite << 30 | 30-bit Morton code of the query
//          clamped into the shape's box, sorted, so a wave gets 64 neighbouring queries.  Where the Morton order jumps
//          across the shape inside a wave, the wave is searched as two parts (mq_split).  Performance devices only.
//   dist   one wave per 64 consecutive sorted queries of one shape.  K = the exact fp32 box of the wave's (or the
//          part's) finite queries.  From there the lattice entry's search with K in place of the brick box
//          (ms_search_bin, the same code): pass 1 finds U = min over bins of the LARGEST box-to-box distance, pass 2
//          searches every other bin whose SMALLEST distance is within U and within the wave's current worst best.
//          The running (best, face) is updated by d < best || (d == best && id < face): the minimum over ALL
//          triangles of one fixed fp64 expression, and the lowest index among its ties, whatever was skipped.  The
//          closest point is evaluated once at the end from the winning face's original vertices.
//   sign   the same waves.  A bin or triangle is a candidate iff its yz-box meets K's yz-box and its lowest x is <= K's
//          highest x; a crossing counts iff x_cross <= (double)q.x; the parity is one bit in a register per lane.  The
//          edge functions, the tie rule and x_cross are the lattice entry's (ms_edge, ms_cross_x).
#include "ofx_tribins.h"

#include <cmath>

#pragma clang fp contract(off)

#include "ofx_tri.h"

namespace {

// the meshes of a call and its queries
struct MqMesh : TbMesh {
  const float* q;
  const int64_t* q_off;
};

// The wave's queries: lane's sorted slot -> query index qi (-1: no query), its point qf and whether it is finite.
__device__ __forceinline__ void mq_wave(const MqMesh& m, const int32_t* __restrict__ sidx, int b, int lane, int64_t& qi,
                                        bool& fin, float (&qf)[3]) {
  const int64_t q0 = m.q_off[b], nq = m.q_off[b + 1] - q0;
  const int64_t s = (int64_t)blockIdx.x * MS_T + lane;
  qi = s < nq ? (int64_t)sidx[q0 + s] : -1;
  fin = qi >= 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    qf[a] = qi >= 0 ? m.q[qi * 3 + a] : 0.f;
    fin = fin && isfinite(qf[a]);
  }
}

// K = the exact box of the points of the lanes with `act` (wave reductions: the same bits in every lane), and its
// squared diagonal.
__device__ __forceinline__ float mq_box(bool act, const float (&qf)[3], float (&klo)[3], float (&khi)[3]) {
  float d2 = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    klo[a] = ms_wave_min(act ? qf[a] : INFINITY);
    khi[a] = ms_wave_max(act ? qf[a] : -INFINITY);
    d2 += (khi[a] - klo[a]) * (khi[a] - klo[a]);
  }
  return d2;
}

// Where to cut the wave in two: the Morton order jumps across the shape now and then, and a wave that holds such a
// jump would search for a box that spans both ends.  The lane after the longest step between consecutive finite
// queries, if the two parts' boxes are together much smaller than the whole (diagonals^2 sum < 1/16); else MS_T, no
// cut.  A performance device only: each part is searched with its own exact box, and the result does not depend on
// the box.  The same value in every lane.
__device__ __forceinline__ int mq_split(bool fin, const float (&qf)[3], int lane) {
  float jump = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float d = qf[a] - __shfl_up(qf[a], 1);
    jump += d * d;
  }
  const bool pfin = __shfl_up((int)fin, 1) != 0;
  jump = (lane > 0 && fin && pfin && jump == jump) ? jump : -1.f;      // (an overflowing step: inf is fine, NaN is not)
  int at = lane;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const float oj = __shfl_xor(jump, s);
    const int oa = __shfl_xor(at, s);
    if (oj > jump || (oj == jump && oa < at)) {
      jump = oj;
      at = oa;
    }
  }
  if (!(jump > 0.f)) return MS_T;
  float lo[3], hi[3];
  const float whole = mq_box(fin, qf, lo, hi);
  const float left = mq_box(fin && lane < at, qf, lo, hi), right = mq_box(fin && lane >= at, qf, lo, hi);
  return (left + right) * 16.f < whole ? at : MS_T;
}

template <bool COUNT>
__global__ __launch_bounds__(MS_T) void mq_dist_kernel(MqMesh m, TbBins w, TbOrder o,
                                                       const int32_t* __restrict__ status, float* __restrict__ dist,
                                                       int32_t* __restrict__ face, float* __restrict__ point,
                                                       unsigned long long* counters) {
  __shared__ double rec[MS_REC * MS_T];
  __shared__ int32_t ids[MS_T];
  uint32_t tally[3] = {0u, 0u, 0u};            // bins searched, triangles staged, triangles evaluated (per wave)
  const int b = blockIdx.y;
  if (status[b]) return;
  if ((int64_t)blockIdx.x * MS_T >= m.q_off[b + 1] - m.q_off[b]) return;
  const int lane = threadIdx.x;
  int64_t qi;
  bool fin;
  float qf[3];
  mq_wave(m, o.sidx, b, lane, qi, fin, qf);
  if (qi >= 0 && !fin) {                        // a non-finite query: NaN, -1, NaN
    dist[qi] = NAN;
    face[qi] = -1;
    if (point) point[qi * 3] = point[qi * 3 + 1] = point[qi * 3 + 2] = NAN;
  }
  const int split = mq_split(fin, qf, lane);
  const int G = tb_G(m, b), G3 = G * G * G;
  const int64_t bin0 = (int64_t)b * m.GS;
#pragma unroll 1
  for (int part = 0; part < 2; ++part) {
    // the part's lanes; any other lane searches for K's low corner (a point of K, so every bound that holds over K
    // holds for it) and writes nothing
    const bool act = fin && (part == 0 ? lane < split : lane >= split);
    if (__ballot(act) == 0ull) continue;
    float klo[3], khi[3];
    mq_box(act, qf, klo, khi);
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = (double)(act ? qf[a] : klo[a]);

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
    int32_t bf = INT32_MAX;
    ms_search_bin<COUNT, true>(w.tri, w.off[bin0 + u_bin], w.off[bin0 + u_bin + 1] - w.off[bin0 + u_bin], lane, klo,
                               khi, p, best, bf, rec, ids, tally);

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
        ms_search_bin<COUNT, true>(w.tri, w.off[bin], w.off[bin + 1] - w.off[bin], lane, klo, khi, p, best, bf, rec,
                                   ids, tally);
      }
    }
    if (act) {
      dist[qi] = (float)sqrt(best);
      face[qi] = bf != INT32_MAX ? bf : -1;         // no finite distance at all (overflow in fp64): no face
      if (point && bf != INT32_MAX) {
        // the winning face again, from its original vertices (valid: the shape's status is 0)
        const int64_t t = m.tri_off[b] + bf, v0 = m.vert_off[b];
        float c[9];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int64_t v = v0 + m.faces[t * 3 + k];
#pragma unroll
          for (int a = 0; a < 3; ++a) c[k * 3 + a] = m.verts[v * 3 + a];
        }
        double cl[3] = {p[0], p[1], p[2]};
        ms_closest(c, p, cl);
#pragma unroll
        for (int a = 0; a < 3; ++a) point[qi * 3 + a] = (float)cl[a];
      }
    }
  }
  if (COUNT && lane < 3) atomicAdd(&counters[lane], (unsigned long long)tally[lane]);
}

__global__ __launch_bounds__(MS_T) void mq_sign_kernel(MqMesh m, TbBins w, TbOrder o,
                                                       const int32_t* __restrict__ status, float* __restrict__ dist) {
  __shared__ double rec[MS_REC * MS_T];
  const int b = blockIdx.y;
  if (status[b]) return;
  if ((int64_t)blockIdx.x * MS_T >= m.q_off[b + 1] - m.q_off[b]) return;
  const int lane = threadIdx.x;
  int64_t qi;
  bool fin;
  float qf[3];
  mq_wave(m, o.sidx, b, lane, qi, fin, qf);
  const int split = mq_split(fin, qf, lane);
  const int G = tb_G(m, b), G3 = G * G * G;
  const int64_t bin0 = (int64_t)b * m.GS;
#pragma unroll 1
  for (int part = 0; part < 2; ++part) {
    const bool act = fin && (part == 0 ? lane < split : lane >= split);
    if (__ballot(act) == 0ull) continue;
    float klo[3], khi[3];
    mq_box(act, qf, klo, khi);
    const double px = (double)(act ? qf[0] : klo[0]), py = (double)(act ? qf[1] : klo[1]);
    const double pz = (double)(act ? qf[2] : klo[2]);
    const double xhi = khi[0], ylo = klo[1], yhi = khi[1], zlo = klo[2], zhi = khi[2];
    uint32_t par = 0u;

    for (int g0 = 0; g0 < G3; g0 += MS_T) {
      const int g = g0 + lane;
      bool cand = false;
      if (g < G3 && w.off[bin0 + g + 1] - w.off[bin0 + g] > 0) {
        float lo[3], hi[3];
        ms_bin_box(w.box, bin0 + g, lo, hi);
        cand = (double)lo[1] <= yhi && (double)hi[1] >= ylo && (double)lo[2] <= zhi && (double)hi[2] >= zlo &&
               (double)lo[0] <= xhi;
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
            for (int q = 0; q < 9; ++q) c[q] = w.tri[(start + t) * TB_W + q];
            const double y0 = c[1], z0 = c[2], y1 = c[4], z1 = c[5], y2 = c[7], z2 = c[8];
            keep = fmin(fmin(y0, y1), y2) <= yhi && fmax(fmax(y0, y1), y2) >= ylo &&
                   fmin(fmin(z0, z1), z2) <= zhi && fmax(fmax(z0, z1), z2) >= zlo &&
                   (double)fminf(fminf(c[0], c[3]), c[6]) <= xhi;      // a crossing is never left of the lowest x
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
            if (s0 == s1 && s1 == s2) par ^= ms_cross_x(rec, q, e01, e20) <= px ? 1u : 0u;
          }
          __syncthreads();
        }
      }
    }
    if (act && par) dist[qi] = -dist[qi];
  }
}

unsigned long long* mq_counters = nullptr;      // ofx_mesh_query_set_counters

}  // namespace

extern "C" size_t ofx_mesh_query_ws_bytes(int batch, int64_t total_verts, int64_t total_faces, int64_t total_q,
                                          int bins) {
  if (!ofx_tribins_args_ok(batch, total_verts, total_faces, total_q, bins)) return 0;
  return ofx_tribins_layout(batch, total_faces, total_q, bins, nullptr, nullptr, nullptr);
}

extern "C" int ofx_mesh_query_set_counters(unsigned long long* words) {
  mq_counters = words;
  return OFX_OK;
}

extern "C" int ofx_mesh_query(const float* verts, const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off,
                              const float* q, const int64_t* q_off, int batch, int64_t total_q, int64_t max_q,
                              int bins, int signed_, float* dist, int32_t* face, float* point, void* ws,
                              int32_t* status, void* stream) {
  if (!verts || !faces || !vert_off || !tri_off || !q_off || !ws || !status ||
      !ofx_tribins_args_ok(batch, 1, 1, total_q, bins) || max_q < 0 || max_q > total_q ||
      (total_q > 0 && (!q || !dist || !face || max_q < 1)))
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  TbBins w;
  TbOrder o;
  ofx_tribins_layout(batch, 0, total_q, bins, (char*)ws, &w, &o);   // the records are last: their size is not needed
  const MqMesh m{{verts, faces, vert_off, tri_off, batch, bins, tb_stride(bins)}, q, q_off};
  int rc = ofx_tribins_build(m, w, total_q, status, stream);
  if (rc || total_q == 0) return rc;              // no queries: the status words are still written
  rc = ofx_tribins_order_points(m, q, q_off, w, o, total_q, stream);
  if (rc) return rc;
  const dim3 waves((unsigned)ofx_cdiv(max_q, MS_T), (unsigned)batch);
  if (mq_counters) mq_dist_kernel<true><<<waves, MS_T, 0, st>>>(m, w, o, status, dist, face, point, mq_counters);
  else mq_dist_kernel<false><<<waves, MS_T, 0, st>>>(m, w, o, status, dist, face, point, nullptr);
  OFX_LAUNCH_CHECK();
  if (signed_) {
    mq_sign_kernel<<<waves, MS_T, 0, st>>>(m, w, o, status, dist);
    OFX_LAUNCH_CHECK();
  }
  return OFX_OK;
}

// The per-shape triangle bins of the point queries and the ray casts (ofx_tribins.h): bound -> count -> ofx_scan_i32 ->
// fill; the fill copies the nine coordinates and the face's index into bin order.  Nothing a search computes depends
// on which bin a triangle is in or on the order inside a bin.  DESIGN.md section 4.19.
#include "ofx_tribins.h"

#include <cmath>

#pragma clang fp contract(off)

#include "ofx_tri.h"

namespace {

__global__ __launch_bounds__(TB_PREP_T) void tb_init_kernel(int64_t nb, TbBins w, int batch,
                                                            int32_t* __restrict__ status) {
  const int64_t stride = (int64_t)gridDim.x * TB_PREP_T;
  for (int64_t i = (int64_t)blockIdx.x * TB_PREP_T + threadIdx.x; i < nb; i += stride) {
    w.cnt[i] = 0;
    w.cursor[i] = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      w.box[i * 6 + a] = INT32_MAX;
      w.box[i * 6 + 3 + a] = INT32_MIN;
    }
    if (i < batch) {
      status[i] = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        w.sbox[i * 6 + a] = INT32_MAX;
        w.sbox[i * 6 + 3 + a] = INT32_MIN;
      }
    }
  }
}

// Bin of a triangle: its centroid in the G^3 grid over the shape's box (a box without extent on an axis: cell 0).
__device__ __forceinline__ int tb_bin_of(const int32_t* __restrict__ sbox, int b, int G, const float (&c)[9]) {
  int g[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double lo = (double)ms_unkey(sbox[b * 6 + a]), ext = (double)ms_unkey(sbox[b * 6 + 3 + a]) - lo;
    const double mid = ((double)c[a] + (double)c[3 + a] + (double)c[6 + a]) * (1.0 / 3.0);
    double f = ext > 0.0 ? floor((mid - lo) / ext * (double)G) : 0.0;
    f = f >= 0.0 ? f : 0.0;                       // written so that a NaN (an overflowing extent) lands in cell 0
    f = f > (double)(G - 1) ? (double)(G - 1) : f;
    g[a] = (int)f;
  }
  return (g[0] * G + g[1]) * G + g[2];
}

// Validate every triangle and bound its shape (min / max on order-preserving keys).  A wave whose triangles all belong
// to one shape reduces its box first: one set of atomics per wave, not per triangle.
__global__ __launch_bounds__(TB_PREP_T) void tb_bound_kernel(TbMesh m, TbBins w, int32_t* __restrict__ status) {
  const int64_t total = m.tri_off[m.batch];
  const int64_t stride = (int64_t)gridDim.x * TB_PREP_T;
  for (int64_t t0 = (int64_t)blockIdx.x * TB_PREP_T; t0 < total; t0 += stride) {      // uniform in a block
    const int64_t t = t0 + threadIdx.x;
    const int b = ms_shape_of(m.tri_off, m.batch, t < total ? t : total - 1);
    float c[9], lo[3], hi[3];
    const bool in = t < total;
    const bool ok = in && ms_load(m.verts, m.faces, m.vert_off, t, b, c);
    if (in && !ok) atomicOr(&status[b], 1);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = ok ? fminf(fminf(c[a], c[3 + a]), c[6 + a]) : INFINITY;
      hi[a] = ok ? fmaxf(fmaxf(c[a], c[3 + a]), c[6 + a]) : -INFINITY;
    }
    const bool one = __shfl(b, 0) == __shfl(b, MS_T - 1);        // shapes are non-decreasing along t
    if (one) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = ms_wave_min(lo[a]);
        hi[a] = ms_wave_max(hi[a]);
      }
    }
    if (one ? ((threadIdx.x & (MS_T - 1)) == 0 && lo[0] <= hi[0]) : ok) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        atomicMin(&w.sbox[b * 6 + a], ms_key(lo[a]));
        atomicMax(&w.sbox[b * 6 + 3 + a], ms_key(hi[a]));
      }
    }
  }
}

// STEP 1: count and bound the bins; 2: copy the records into bin order.
template <int STEP>
__global__ __launch_bounds__(TB_PREP_T) void tb_bin_kernel(TbMesh m, TbBins w) {
  const int64_t total = m.tri_off[m.batch];
  const int64_t stride = (int64_t)gridDim.x * TB_PREP_T;
  for (int64_t t = (int64_t)blockIdx.x * TB_PREP_T + threadIdx.x; t < total; t += stride) {
    const int b = ms_shape_of(m.tri_off, m.batch, t);
    float c[9];
    if (!ms_load(m.verts, m.faces, m.vert_off, t, b, c)) continue;      // tb_bound_kernel has set the status
    const int64_t bin = (int64_t)b * m.GS + tb_bin_of(w.sbox, b, tb_G(m, b), c);
    if (STEP == 1) {
      atomicAdd(&w.cnt[bin], 1);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        atomicMin(&w.box[bin * 6 + a], ms_key(fminf(fminf(c[a], c[3 + a]), c[6 + a])));
        atomicMax(&w.box[bin * 6 + 3 + a], ms_key(fmaxf(fmaxf(c[a], c[3 + a]), c[6 + a])));
      }
    } else {
      const int64_t slot = (int64_t)w.off[bin] + atomicAdd(&w.cursor[bin], 1);
#pragma unroll
      for (int k = 0; k < 9; ++k) w.tri[slot * TB_W + k] = c[k];
      w.tri[slot * TB_W + 9] = __int_as_float((int32_t)(t - m.tri_off[b]));
    }
  }
}

// Sort key of every point: shape << 32 | non-finite << 30 | Morton code of the point in a 1024^3 grid over the shape's
// box.  Only the shape bits matter for a result (a shape's points stay in its range of sorted positions).
__global__ __launch_bounds__(TB_PREP_T) void tb_key_kernel(int batch, const float* __restrict__ q,
                                                           const int64_t* __restrict__ q_off, TbBins w, TbOrder o,
                                                           int64_t total_q) {
  const int64_t stride = (int64_t)gridDim.x * TB_PREP_T;
  for (int64_t i = (int64_t)blockIdx.x * TB_PREP_T + threadIdx.x; i < total_q; i += stride) {
    const int b = ms_shape_of(q_off, batch, i);
    uint64_t code = 0;
    bool fin = true;
    int cell[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float v = q[i * 3 + a];
      fin = fin && isfinite(v);
      const float lo = ms_unkey(w.sbox[b * 6 + a]), ext = ms_unkey(w.sbox[b * 6 + 3 + a]) - lo;
      const float f = (v - lo) / ext * 1024.f;
      cell[a] = f >= 0.f ? (f < 1023.f ? (int)f : 1023) : 0;      // a NaN lands in cell 0
    }
    code = fin ? ofx_xyz2morton(cell[0], cell[1], cell[2]) : (1ull << 30);
    o.key[i] = (int64_t)(((uint64_t)b << 32) | code);
    o.idx[i] = (int32_t)i;
  }
}

}  // namespace

bool ofx_tribins_args_ok(int batch, int64_t total_verts, int64_t total_faces, int64_t total_q, int bins) {
  return batch >= 1 && batch <= 65535 && total_verts >= 1 && total_faces >= 1 && total_faces <= INT32_MAX &&
         total_q >= 0 && total_q <= (int64_t(1) << 30) && bins >= 0 && bins <= TB_MAX_G;
}

size_t ofx_tribins_layout(int batch, int64_t total_faces, int64_t total_q, int bins, char* base, TbBins* w,
                          TbOrder* o) {
  const int64_t nb = (int64_t)batch * tb_stride(bins);
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + at : nullptr;
    at += tb_align(bytes);
    return p;
  };
  TbBins l;
  TbOrder s;
  l.cnt = (int32_t*)take(nb * sizeof(int32_t));
  l.off = (int32_t*)take((nb + 1) * sizeof(int32_t));
  l.cursor = (int32_t*)take(nb * sizeof(int32_t));
  l.box = (int32_t*)take(nb * 6 * sizeof(int32_t));
  l.sbox = (int32_t*)take((size_t)batch * 6 * sizeof(int32_t));
  l.scan_ws = take(ofx_scan_ws_bytes(nb));
  s.key = (int64_t*)take((size_t)total_q * sizeof(int64_t));
  s.skey = (int64_t*)take((size_t)total_q * sizeof(int64_t));
  s.idx = (int32_t*)take((size_t)total_q * sizeof(int32_t));
  s.sidx = (int32_t*)take((size_t)total_q * sizeof(int32_t));
  s.sort_bytes = ofx_points_sort_ws_bytes(total_q);
  s.sort_ws = take(s.sort_bytes);
  l.tri = (float*)take((size_t)total_faces * TB_W * sizeof(float));
  if (w) *w = l;
  if (o) *o = s;
  return at;
}

int ofx_tribins_build(const TbMesh& m, const TbBins& w, int64_t total_q, int32_t* status, void* stream) {
  hipStream_t st = ofx_stream(stream);
  const int64_t nb = (int64_t)m.batch * m.GS;
  tb_init_kernel<<<ofx_grid(nb, TB_PREP_T), TB_PREP_T, 0, st>>>(nb, w, m.batch, status);
  OFX_LAUNCH_CHECK();
  const int prep = 2048;                          // grid-stride: the face count lives on the device
  tb_bound_kernel<<<prep, TB_PREP_T, 0, st>>>(m, w, status);
  OFX_LAUNCH_CHECK();
  if (total_q == 0) return OFX_OK;                // the status words are still written
  tb_bin_kernel<1><<<prep, TB_PREP_T, 0, st>>>(m, w);
  OFX_LAUNCH_CHECK();
  const int rc = ofx_scan_i32(w.cnt, w.off, nb, w.scan_ws, stream);
  if (rc) return rc;
  tb_bin_kernel<2><<<prep, TB_PREP_T, 0, st>>>(m, w);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

int ofx_tribins_order_points(const TbMesh& m, const float* q, const int64_t* q_off, const TbBins& w, const TbOrder& o,
                             int64_t total_q, void* stream) {
  tb_key_kernel<<<ofx_grid(total_q, TB_PREP_T), TB_PREP_T, 0, ofx_stream(stream)>>>(m.batch, q, q_off, w, o, total_q);
  OFX_LAUNCH_CHECK();
  return ofx_points_sort(o.key, o.idx, total_q, o.skey, o.sidx, o.sort_ws, o.sort_bytes, stream);
}

// Evaluation metrics of generated shapes: surface sampling, the directed nearest-neighbour (Chamfer) matrix and the
// approximate-EMD matrix.  The reference scores samples with its metrics/ package: trimesh sampling after
// scale_to_unit_cube (metrics/generate_pointclouds.py:14-37), nndistance.cu for Chamfer and approxmatch.cu
// (approxmatchkernel + matchcostkernel, :3-224) for EMD, driven one sample at a time against 256-shape batches
// (metrics/evaluation_metrics.py:111-153).  Here every kernel covers a whole matrix in one launch.
//
// Contract (include/ofx.h; restated in float64 by tests/metrics_oracle.py):
//   sampling  per shape: bounding box of the vertices, optional normalisation (v - centre) * 2 / max extent; twice
//             the triangle areas in fp64, an fp64 inclusive prefix per shape (one block per shape, fixed order:
//             bitwise reproducible); point i of shape s draws r_d = hash(seed, id_s, i, d), d = 0, 1, 2: triangle =
//             first t with prefix[t] > (r_0 >> 11) * 2^-53 * total, barycentrics u = (r_1 >> 40) * 2^-24,
//             w = (r_2 >> 40) * 2^-24, reflected to (1 - u, 1 - w) when (r_1 >> 40) + (r_2 >> 40) > 2^24;
//             p = A + u (B - A) + w (C - A) on the normalised vertices.
//             The oriented entry point adds the unit normal (B - A) x (C - A) / |.| of the drawn triangle, in fp64 from
//             the raw vertices, rounded once (same kernel body: sp_sample_kernel<true>).
//   NN        D[a, b] = mean_p min_q |p - q|^2, p over A[a], q over B[b], direct differences (a cloud against itself
//             gives exactly 0).  Queries live in registers (8 per lane, packed in pairs: v_pk_* f32), targets stream
//             through LDS as broadcast (x, y, z, .) reads, one block owns one query cloud and NN_BT target clouds.
//   EMD       one block per ordered cloud pair (X[a] as xyz1, Y[b] as xyz2); both clouds sit in LDS as float4
//             (x, y, z, ratio); remainL / remainR / ratioL stay in the registers of the lane that owns the point;
//             the match cost is fused into the third pass, so the n x m match matrix is never stored.
#include "ofx_common.h"

#include <cmath>

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------------ surface sampling
// (the counter hash mt_step lives in ofx_common.h: csrc/ofx_sdfdata.hip draws from it too)
constexpr int SP_T = 1024;                 // prep: one block per shape

// Block-wide inclusive scan of a double in thread order; `total` = the block sum.  All threads must call it.
__device__ __forceinline__ double sp_block_scan(double x, double* lds, double& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) lds[wave] = x;
  __syncthreads();
  double before = 0.0;
  total = 0.0;
#pragma unroll
  for (int w = 0; w < SP_T / 64; ++w) {
    const double t = lds[w];
    before += w < wave ? t : 0.0;
    total += t;
  }
  __syncthreads();
  return before + x;
}

__global__ __launch_bounds__(SP_T) void sp_prep_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                       const int64_t* __restrict__ offs, int batch, int normalize,
                                                       float* __restrict__ frame, double* __restrict__ cdf) {
  __shared__ float red[6][SP_T / 64];
  __shared__ double lds[SP_T / 64];
  const int b = blockIdx.x;
  const int64_t voff = offs[b], nv = offs[batch + b], foff = offs[2 * batch + b], nf = offs[3 * batch + b];
  const float* v = verts + voff * 3;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = threadIdx.x; i < nv; i += SP_T) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float c = v[i * 3 + a];
      mn[a] = fminf(mn[a], c);
      mx[a] = fmaxf(mx[a], c);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], o));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o));
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      red[a][wave] = mn[a];
      red[3 + a][wave] = mx[a];
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = red[a][0];
      hi[a] = red[3 + a][0];
      for (int w = 1; w < SP_T / 64; ++w) {
        lo[a] = fminf(lo[a], red[a][w]);
        hi[a] = fmaxf(hi[a], red[3 + a][w]);
      }
    }
    float c[3] = {0.f, 0.f, 0.f}, s = 1.f;
    if (normalize && nv > 0) {
      float ext = 0.f;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        c[a] = __fmul_rn(__fadd_rn(lo[a], hi[a]), 0.5f);
        ext = fmaxf(ext, __fsub_rn(hi[a], lo[a]));
      }
      s = ext > 0.f ? __fdiv_rn(2.f, ext) : 1.f;
    }
    float* fr = frame + (int64_t)b * 4;
    fr[0] = c[0];
    fr[1] = c[1];
    fr[2] = c[2];
    fr[3] = s;
  }
  // twice the triangle areas (raw coordinates: normalising scales every area alike), fp64 prefix in face order
  const int32_t* f = faces + foff * 3;
  double* out = cdf + foff;
  double carry = 0.0;
  for (int64_t base = 0; base < nf; base += SP_T) {
    const int64_t i = base + threadIdx.x;
    double area = 0.0;
    if (i < nf) {
      const float* p0 = v + (int64_t)f[i * 3 + 0] * 3;
      const float* p1 = v + (int64_t)f[i * 3 + 1] * 3;
      const float* p2 = v + (int64_t)f[i * 3 + 2] * 3;
      const double ax = (double)p1[0] - p0[0], ay = (double)p1[1] - p0[1], az = (double)p1[2] - p0[2];
      const double bx = (double)p2[0] - p0[0], by = (double)p2[1] - p0[1], bz = (double)p2[2] - p0[2];
      const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
      area = sqrt(cx * cx + cy * cy + cz * cz);
    }
    double total;
    const double incl = sp_block_scan(area, lds, total);
    if (i < nf) out[i] = carry + incl;
    carry += total;
  }
}

// ORIENTED: also write the unit normal (B - A) x (C - A) / |.| of the drawn triangle, from the raw vertices (the
// normalisation is a positive scale and a translation: same direction, one rounding less).  The differences of fp32
// coordinates are exact in fp64, so the normal is the fp32 rounding of the true one however thin the triangle is.
// The draw itself -- hash, prefix search, barycentrics, point -- is this one body for both instantiations.
template <bool ORIENTED>
__global__ void sp_sample_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                 const int64_t* __restrict__ offs, const int64_t* __restrict__ ids, int batch, int n,
                                 uint64_t seed, const float* __restrict__ frame, const double* __restrict__ cdf,
                                 float* __restrict__ out, float* __restrict__ normals) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (int64_t)batch * n) return;
  const int b = (int)(g / n), i = (int)(g % n);
  const int64_t voff = offs[b], foff = offs[2 * batch + b], nf = offs[3 * batch + b];
  float* o = out + g * 3;
  if (nf <= 0) {                                  // the caller refuses such shapes; never read an empty prefix
    o[0] = o[1] = o[2] = NAN;
    if constexpr (ORIENTED) normals[g * 3 + 0] = normals[g * 3 + 1] = normals[g * 3 + 2] = NAN;
    return;
  }
  const double* c = cdf + foff;
  const uint64_t h = mt_step(mt_step(seed, ids ? (uint64_t)ids[b] : (uint64_t)b), (uint64_t)i);
  const uint64_t r0 = mt_step(h, 0), r1 = mt_step(h, 1), r2 = mt_step(h, 2);
  const double target = (double)(r0 >> 11) * 0x1p-53 * c[nf - 1];
  int64_t lo = 0, hi = nf - 1;                    // first t with c[t] > target (the last one if none)
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (c[mid] > target) hi = mid;
    else lo = mid + 1;
  }
  uint32_t iu = (uint32_t)(r1 >> 40), iw = (uint32_t)(r2 >> 40);
  if (iu + iw > (1u << 24)) {
    iu = (1u << 24) - iu;
    iw = (1u << 24) - iw;
  }
  const float u = (float)iu * 0x1p-24f, w = (float)iw * 0x1p-24f;
  const float* fr = frame + (int64_t)b * 4;
  const int32_t* tri = faces + (foff + lo) * 3;
  const float* v = verts + voff * 3;
  float raw[3][3], p[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float* q = v + (int64_t)tri[k] * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      raw[k][a] = q[a];
      p[k][a] = __fmul_rn(__fsub_rn(raw[k][a], fr[a]), fr[3]);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
    o[a] = __fadd_rn(__fadd_rn(p[0][a], __fmul_rn(u, __fsub_rn(p[1][a], p[0][a]))),
                     __fmul_rn(w, __fsub_rn(p[2][a], p[0][a])));
  if constexpr (ORIENTED) {
    const double ax = (double)raw[1][0] - raw[0][0], ay = (double)raw[1][1] - raw[0][1], az = (double)raw[1][2] - raw[0][2];
    const double bx = (double)raw[2][0] - raw[0][0], by = (double)raw[2][1] - raw[0][1], bz = (double)raw[2][2] - raw[0][2];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const double len = sqrt(cx * cx + cy * cy + cz * cz);
    const double inv = len > 0.0 ? 1.0 / len : 0.0;      // only a shape of total area 0 can draw such a triangle
    float* nm = normals + g * 3;
    nm[0] = (float)(cx * inv);
    nm[1] = (float)(cy * inv);
    nm[2] = (float)(cz * inv);
  }
}

struct SpWs {
  float* frame;   // [batch][4]  centre x, y, z, scale
  double* cdf;    // [total_faces]
};

inline size_t sp_align(size_t b) { return (b + 255) & ~(size_t)255; }

size_t sp_layout(int batch, int64_t total_faces, char* base, SpWs* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += sp_align(bytes);
    return p;
  };
  SpWs l;
  l.frame = (float*)take((size_t)batch * 4 * sizeof(float));
  l.cdf = (double*)take((size_t)(total_faces > 0 ? total_faces : 1) * sizeof(double));
  if (w) *w = l;
  return off;
}

// ------------------------------------------------------------------------------------------------ NN matrix
constexpr int NN_T = 256;                  // threads per block (4 waves)
constexpr int NN_Q = 8;                    // query points per lane, four packed pairs
constexpr int NN_QCHUNK = NN_T * NN_Q;     // query points per register pass (2048: one reference cloud)
constexpr int NN_TILE = 1024;              // target points per LDS tile (16 KiB)
constexpr int NN_BT = 4;                   // target clouds per block

__global__ __launch_bounds__(NN_T) void nn_kernel(const float* __restrict__ A, int n, const float* __restrict__ B,
                                                  int64_t nb, int m, int64_t ntile_b, float* __restrict__ D) {
  __shared__ float4 tile[NN_TILE];
  __shared__ float red[NN_BT][NN_T / 64];
  const int64_t a = blockIdx.x / ntile_b;
  const int64_t b0 = (blockIdx.x % ntile_b) * NN_BT;
  const int nbt = (int)(nb - b0 < NN_BT ? nb - b0 : NN_BT);
  const float* qa = A + a * (int64_t)n * 3;
  const int tid = threadIdx.x;
  float sum[NN_BT];
#pragma unroll
  for (int t = 0; t < NN_BT; ++t) sum[t] = 0.f;

  for (int q0 = 0; q0 < n; q0 += NN_QCHUNK) {
    f2 qx[NN_Q / 2], qy[NN_Q / 2], qz[NN_Q / 2];
#pragma unroll
    for (int j = 0; j < NN_Q; ++j) {
      const int q = q0 + j * NN_T + tid;
      float x = 0.f, y = 0.f, z = 0.f;
      if (q < n) {
        x = qa[(int64_t)q * 3 + 0];
        y = qa[(int64_t)q * 3 + 1];
        z = qa[(int64_t)q * 3 + 2];
      }
      qx[j >> 1][j & 1] = x;
      qy[j >> 1][j & 1] = y;
      qz[j >> 1][j & 1] = z;
    }
#pragma unroll
    for (int bt = 0; bt < NN_BT; ++bt) {
      if (bt >= nbt) break;                        // uniform over the block
      const float* tb = B + (b0 + bt) * (int64_t)m * 3;
      f2 mn[NN_Q / 2];
#pragma unroll
      for (int p = 0; p < NN_Q / 2; ++p) mn[p] = f2{INFINITY, INFINITY};
#pragma unroll 1
      for (int t0 = 0; t0 < m; t0 += NN_TILE) {
        const int cnt = m - t0 < NN_TILE ? m - t0 : NN_TILE;
        const int cnt2 = (cnt + 1) & ~1;          // pairs of targets; the odd slot is padded with +inf
        __syncthreads();
        for (int i = tid; i < cnt2; i += NN_T) {
          float4 s = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
          if (i < cnt) {
            const float* src = tb + (int64_t)(t0 + i) * 3;
            s = make_float4(src[0], src[1], src[2], 0.f);
          }
          tile[i] = s;
        }
        __syncthreads();
#pragma unroll 2
        for (int l = 0; l < cnt2; l += 2) {
          const float4 s0 = tile[l], s1 = tile[l + 1];
#pragma unroll
          for (int p = 0; p < NN_Q / 2; ++p) {
            const f2 dx0 = qx[p] - s0.x, dy0 = qy[p] - s0.y, dz0 = qz[p] - s0.z;
            const f2 dx1 = qx[p] - s1.x, dy1 = qy[p] - s1.y, dz1 = qz[p] - s1.z;
            const f2 d0 = dz0 * dz0 + (dy0 * dy0 + dx0 * dx0);
            const f2 d1 = dz1 * dz1 + (dy1 * dy1 + dx1 * dx1);
            mn[p].x = fminf(mn[p].x, fminf(d0.x, d1.x));
            mn[p].y = fminf(mn[p].y, fminf(d0.y, d1.y));
          }
        }
      }
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < NN_Q; ++j)
        if (q0 + j * NN_T + tid < n) s += mn[j >> 1][j & 1];
      sum[bt] += s;
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int t = 0; t < NN_BT; ++t) {
    float s = sum[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) red[t][wave] = s;
  }
  __syncthreads();
  if (tid < nbt) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NN_T / 64; ++w) s += red[tid][w];
    D[a * nb + b0 + tid] = s / (float)n;
  }
}

// ------------------------------------------------------------------------------------------------ EMD matrix
constexpr int EM_T = 512;                  // threads per block (8 waves)
constexpr int EM_P = 4;                    // points each lane owns, as a row (xyz1) and as a column (xyz2)
constexpr int EM_MAX = EM_T * EM_P;        // 2048: both clouds as float4 in LDS = 64 KiB, two blocks per CU
constexpr float EM_LOG2E = 1.44269504088896341f;
static_assert(EM_MAX == OFX_EMD_MAX_POINTS, "include/ofx.h documents the limit");

__device__ __forceinline__ f2 em_exp2(f2 x) { return f2{__builtin_amdgcn_exp2f(x.x), __builtin_amdgcn_exp2f(x.y)}; }
__device__ __forceinline__ f2 em_sqrt(f2 x) { return f2{__builtin_amdgcn_sqrtf(x.x), __builtin_amdgcn_sqrtf(x.y)}; }

__global__ __launch_bounds__(EM_T) void emd_kernel(const float* __restrict__ X, const float* __restrict__ Y, int64_t ny,
                                                   int n, float* __restrict__ E) {
  extern __shared__ float4 em_lds[];
  float4* P1 = em_lds;                     // xyz1, .w = ratioL
  float4* P2 = em_lds + n;                 // xyz2, .w = remainR (pass 1) / ratioR (pass 3)
  __shared__ float red[EM_T / 64];
  const int64_t a = blockIdx.x / ny, b = blockIdx.x % ny;
  const float* x1 = X + a * (int64_t)n * 3;
  const float* x2 = Y + b * (int64_t)n * 3;
  const int tid = threadIdx.x;

  f2 kx[EM_P / 2], ky[EM_P / 2], kz[EM_P / 2];   // owned rows (xyz1)
  f2 lx[EM_P / 2], ly[EM_P / 2], lz[EM_P / 2];   // owned columns (xyz2)
  float remL[EM_P], remR[EM_P], ratL[EM_P], cost[EM_P];
#pragma unroll
  for (int j = 0; j < EM_P; ++j) {
    const int k = tid + j * EM_T;
    float p[3] = {0.f, 0.f, 0.f}, q[3] = {0.f, 0.f, 0.f};
    if (k < n) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        p[c] = x1[(int64_t)k * 3 + c];
        q[c] = x2[(int64_t)k * 3 + c];
      }
      P1[k] = make_float4(p[0], p[1], p[2], 0.f);
      P2[k] = make_float4(q[0], q[1], q[2], 0.f);
    }
    kx[j >> 1][j & 1] = p[0];
    ky[j >> 1][j & 1] = p[1];
    kz[j >> 1][j & 1] = p[2];
    lx[j >> 1][j & 1] = q[0];
    ly[j >> 1][j & 1] = q[1];
    lz[j >> 1][j & 1] = q[2];
    remL[j] = 1.f;                       // n == m: multiL = multiR = 1
    remR[j] = 1.f;
    ratL[j] = 0.f;
    cost[j] = 0.f;
  }

#pragma unroll 1
  for (int lev = 7; lev >= -1; --lev) {      // levels -4^j, j = 7 .. -1 (the reference's j == -2 branch never runs)
    const float c2 = -ldexpf(1.f, 2 * lev) * EM_LOG2E;     // exp(level * d2) = exp2(c2 * d2)
#pragma unroll
    for (int j = 0; j < EM_P; ++j) {
      const int k = tid + j * EM_T;
      if (k < n) P2[k].w = remR[j];
    }
    __syncthreads();
    // pass 1: row sums -> ratioL
    {
      f2 s[EM_P / 2];
#pragma unroll
      for (int j = 0; j < EM_P / 2; ++j) s[j] = f2{1e-9f, 1e-9f};
#pragma unroll 2
      for (int l = 0; l < n; ++l) {
        const float4 q = P2[l];
#pragma unroll
        for (int j = 0; j < EM_P / 2; ++j) {
          const f2 dx = kx[j] - q.x, dy = ky[j] - q.y, dz = kz[j] - q.z;
          s[j] += em_exp2(c2 * (dz * dz + (dy * dy + dx * dx))) * q.w;
        }
      }
#pragma unroll
      for (int j = 0; j < EM_P; ++j) {
        ratL[j] = remL[j] / s[j >> 1][j & 1];
        const int k = tid + j * EM_T;
        if (k < n) P1[k].w = ratL[j];
      }
    }
    __syncthreads();
    // pass 2: column sums -> ratioR, remainR
    {
      f2 s[EM_P / 2];
#pragma unroll
      for (int j = 0; j < EM_P / 2; ++j) s[j] = f2{0.f, 0.f};
#pragma unroll 2
      for (int k = 0; k < n; ++k) {
        const float4 p = P1[k];
#pragma unroll
        for (int j = 0; j < EM_P / 2; ++j) {
          const f2 dx = lx[j] - p.x, dy = ly[j] - p.y, dz = lz[j] - p.z;
          s[j] += em_exp2(c2 * (dz * dz + (dy * dy + dx * dx))) * p.w;
        }
      }
#pragma unroll
      for (int j = 0; j < EM_P; ++j) {
        const float sumr = s[j >> 1][j & 1] * remR[j];
        const float consumption = fminf(remR[j] / (sumr + 1e-9f), 1.f);
        const float ratR = consumption * remR[j];
        remR[j] = fmaxf(0.f, remR[j] - sumr);
        const int l = tid + j * EM_T;
        if (l < n) P2[l].w = ratR;
      }
    }
    __syncthreads();
    // pass 3: match increment (ratioL[k] factored out of the row) fused with its cost, remainL update
    {
      f2 s[EM_P / 2], cs[EM_P / 2];
#pragma unroll
      for (int j = 0; j < EM_P / 2; ++j) s[j] = cs[j] = f2{0.f, 0.f};
#pragma unroll 2
      for (int l = 0; l < n; ++l) {
        const float4 q = P2[l];
#pragma unroll
        for (int j = 0; j < EM_P / 2; ++j) {
          const f2 dx = kx[j] - q.x, dy = ky[j] - q.y, dz = kz[j] - q.z;
          const f2 d2 = dz * dz + (dy * dy + dx * dx);
          const f2 w = em_exp2(c2 * d2) * q.w;
          s[j] += w;
          cs[j] += w * em_sqrt(d2);
        }
      }
#pragma unroll
      for (int j = 0; j < EM_P; ++j) {
        const float suml = ratL[j] * s[j >> 1][j & 1];
        cost[j] += ratL[j] * cs[j >> 1][j & 1];
        remL[j] = fmaxf(0.f, remL[j] - suml);
      }
    }
    __syncthreads();
  }
  float t = 0.f;
#pragma unroll
  for (int j = 0; j < EM_P; ++j)
    if (tid + j * EM_T < n) t += cost[j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  if ((tid & 63) == 0) red[tid >> 6] = t;
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < EM_T / 64; ++w) s += red[w];
    E[blockIdx.x] = s / (float)n;
  }
}

bool emd_lds_done[OFX_MAX_DEVICES];

}  // namespace

extern "C" size_t ofx_surface_sample_ws_bytes(int batch, int64_t total_faces) {
  if (batch < 1 || total_faces < 1) return 0;
  return sp_layout(batch, total_faces, nullptr, nullptr);
}

namespace {

int sp_run(const float* verts, const int32_t* faces, const int64_t* offs, const int64_t* ids, int batch,
           int64_t total_faces, int n, uint64_t seed, int normalize, void* ws, float* out, float* normals, void* stream) {
  if (!verts || !faces || !offs || !ws || !out || batch < 1 || n < 1 || total_faces < 1 ||
      ofx_cdiv((int64_t)batch * n, 256) > INT32_MAX)
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  SpWs w;
  sp_layout(batch, total_faces, (char*)ws, &w);
  sp_prep_kernel<<<batch, SP_T, 0, st>>>(verts, faces, offs, batch, normalize ? 1 : 0, w.frame, w.cdf);
  OFX_LAUNCH_CHECK();
  const unsigned grid = (unsigned)ofx_cdiv((int64_t)batch * n, 256);
  if (normals)
    sp_sample_kernel<true><<<grid, 256, 0, st>>>(verts, faces, offs, ids, batch, n, seed, w.frame, w.cdf, out, normals);
  else
    sp_sample_kernel<false><<<grid, 256, 0, st>>>(verts, faces, offs, ids, batch, n, seed, w.frame, w.cdf, out, nullptr);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

}  // namespace

extern "C" int ofx_surface_sample(const float* verts, const int32_t* faces, const int64_t* offs, const int64_t* ids,
                                  int batch, int64_t total_faces, int n, uint64_t seed, int normalize, void* ws,
                                  float* out, void* stream) {
  return sp_run(verts, faces, offs, ids, batch, total_faces, n, seed, normalize, ws, out, nullptr, stream);
}

extern "C" int ofx_surface_sample_oriented(const float* verts, const int32_t* faces, const int64_t* offs,
                                           const int64_t* ids, int batch, int64_t total_faces, int n, uint64_t seed,
                                           int normalize, void* ws, float* out, float* normals, void* stream) {
  if (!normals) return OFX_EINVAL;
  return sp_run(verts, faces, offs, ids, batch, total_faces, n, seed, normalize, ws, out, normals, stream);
}

extern "C" int ofx_nn_matrix(const float* a, int64_t na, int n, const float* b, int64_t nb, int m, float* d,
                             void* stream) {
  if (!a || !b || !d || na < 1 || nb < 1 || n < 1 || m < 1) return OFX_EINVAL;
  const int64_t ntile_b = ofx_cdiv(nb, NN_BT);
  if (na * ntile_b > INT32_MAX) return OFX_EINVAL;
  nn_kernel<<<(unsigned)(na * ntile_b), NN_T, 0, ofx_stream(stream)>>>(a, n, b, nb, m, ntile_b, d);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" int ofx_emd_matrix(const float* x, int64_t nx, const float* y, int64_t ny, int n, int m, float* e,
                              void* stream) {
  if (!x || !y || !e || nx < 1 || ny < 1 || n < 1 || n != m || n > OFX_EMD_MAX_POINTS || nx * ny > INT32_MAX)
    return OFX_EINVAL;
  if (!ofx_raise_lds_limit((const void*)emd_kernel, 2 * EM_MAX * (int)sizeof(float4), emd_lds_done)) return OFX_ELAUNCH;
  emd_kernel<<<(unsigned)(nx * ny), EM_T, 2 * n * sizeof(float4), ofx_stream(stream)>>>(x, y, ny, n, e);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" uint64_t ofx_metrics_hash(uint64_t seed, int64_t shape, int64_t point, int draw) {
  return mt_step(mt_step(mt_step(seed, (uint64_t)shape), (uint64_t)point), (uint64_t)draw);
}

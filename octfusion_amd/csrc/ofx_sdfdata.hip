// Training samples of the GraphVAE drawn from an SDF lattice: the reference's tools/repair_mesh.py sample_sdf
// (:293-334: k random points in every octree node of depths full_depth..depth, trilinear value and normalised
// central-difference gradient, torch fp32 on the host) and sample_occu (:358-375: uniform points, trilinear value in
// numpy fp64, packed occupancy bits).
//
// Contract (include/ofx.h; restated with numpy by tests/sdfdata_oracle.py).  The lattice is sdf[(x*S + y)*S + z] fp32.
//   nodes  candidate g = i*k + j is sample j of node i (nodes of all depths concatenated, depth-major; the depth of
//          node i is depth_start + the segment of depth_off it falls in).  p = fl32(fl32(node + u) * fl32(S * 2^-d)),
//          kept iff 0 <= p < S - 1 on all three axes (the reference's test is the upper one; the lower one only turns
//          away inputs the reference cannot produce, and keeps every read inside the lattice).  Corners in the
//          reference's `grid` order c = dx*4 + dy*2 + dz, weights ((1-|fx|) * (1-|fy|)) * (1-|fz|) and their sum in
//          that order, the three gradient sums left to right as the reference writes them, all fp32, no contraction.
//   order  kept samples are written in candidate order.  Count pass: one ballot per wave, one count per block;
//          ofx_scan_i32 over the block counts; emit pass: slot = block prefix + waves before + lanes before.  No atomics:
//          the output is bitwise reproducible.
//   occu   point i: pu = u * ((S-1)/S), q = pu * S, trilinear value in fp64 over the fp32 corners, the eight products
//          summed pairwise (numpy's order for a row of eight); bit = value < 0.  One ballot per wave; the lane of every
//          eighth point reverses its byte of the ballot (numpy.packbits: first point in the top bit) and stores it.
//   fp16   round to nearest even, once: fp32 values through the hardware conversion, fp64 values through a
//          round-to-odd fp32 intermediate (13 spare bits: the second rounding sees exactly what the first one lost).
#include "ofx_common.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int SD_T = 256;          // threads per block (4 waves), one candidate sample each

__device__ __forceinline__ uint16_t sd_half(float f) {
  const _Float16 h = (_Float16)f;  // v_cvt_f16_f32: round to nearest even
  return __builtin_bit_cast(uint16_t, h);
}
__device__ __forceinline__ float sd_unhalf(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }

// fp64 -> fp16, correctly rounded: truncate to fp32 toward zero, set the last bit if anything was lost, round once.
__device__ __forceinline__ uint16_t sd_half(double d) {
  float f = (float)d;
  if ((double)f != d) {
    uint32_t b = __float_as_uint(f);
    if (fabs((double)f) > fabs(d)) b -= 1;      // |f| > |d| > 0: f is not +-0, so the step stays in the same sign
    f = __uint_as_float(b | 1u);
  }
  return sd_half(f);
}

struct SdNodes {
  const float* sdf;
  const int32_t* xyz;
  const int64_t* depth_off;
  const float* u;
  int64_t total;                   // N * k candidates
  int S, n_depths, depth_start, k;
  uint64_t seed;
  int64_t shape;
};

// Position of candidate g on the lattice; true iff it is kept.
__device__ __forceinline__ bool sd_position(const SdNodes& a, int64_t g, float (&p)[3]) {
  const int64_t i = g / a.k;
  int seg = 0;
  for (int s = 1; s < a.n_depths; ++s) seg += i >= a.depth_off[s] ? 1 : 0;
  const float scale = ldexpf((float)a.S, -(a.depth_start + seg));
  const float top = (float)(a.S - 1);
  bool keep = true;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float u;
    if (a.u) u = a.u[g * 3 + c];
    else u = (float)(uint32_t)(mt_step(mt_step(mt_step(a.seed, (uint64_t)a.shape), (uint64_t)g), (uint64_t)c) >> 40) * 0x1p-24f;
    p[c] = ((float)a.xyz[i * 3 + c] + u) * scale;
    keep = keep && p[c] >= 0.f && p[c] < top;
  }
  return keep;
}

__global__ __launch_bounds__(SD_T) void sd_count_kernel(SdNodes a, int32_t* __restrict__ cnt) {
  __shared__ int32_t wcnt[SD_T / 64];
  const int64_t g = (int64_t)blockIdx.x * SD_T + threadIdx.x;
  float p[3];
  const bool keep = g < a.total && sd_position(a, g, p);
  const uint64_t m = __ballot(keep);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t s = 0;
#pragma unroll
    for (int w = 0; w < SD_T / 64; ++w) s += wcnt[w];
    cnt[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(SD_T) void sd_emit_kernel(SdNodes a, const int32_t* __restrict__ pre, float shape_scale,
                                                       uint16_t* __restrict__ points, uint16_t* __restrict__ grad,
                                                       uint16_t* __restrict__ val, int64_t* __restrict__ count) {
  __shared__ int32_t wcnt[SD_T / 64];
  const int64_t g = (int64_t)blockIdx.x * SD_T + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float p[3];
  const bool keep = g < a.total && sd_position(a, g, p);
  const uint64_t m = __ballot(keep);
  if (lane == 0) wcnt[wave] = __popcll(m);
  __syncthreads();
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *count = pre[gridDim.x];
  if (!keep) return;
  int64_t slot = pre[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) slot += wcnt[w];

  int xi[3];
  float f0[3], f1[3];               // |p - corner| toward the lower and the upper corner
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float fl = floorf(p[c]);
    xi[c] = (int)fl;                // 0 <= xi <= S - 2: p < S - 1
    f0[c] = fabsf(p[c] - fl);
    f1[c] = fabsf(p[c] - (fl + 1.f));
  }
  const int S = a.S;
  float s[8];
#pragma unroll
  for (int q = 0; q < 4; ++q) {     // the two z-neighbours of a corner pair are adjacent in memory
    const float* row = a.sdf + ((int64_t)(xi[0] + (q >> 1)) * S + (xi[1] + (q & 1))) * S + xi[2];
    s[2 * q] = row[0];
    s[2 * q + 1] = row[1];
  }
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float wx = 1.f - ((c & 4) ? f1[0] : f0[0]);
    const float wy = 1.f - ((c & 2) ? f1[1] : f0[1]);
    const float wz = 1.f - ((c & 1) ? f1[2] : f0[2]);
    v = v + s[c] * ((wx * wy) * wz);
  }
  const float gx = s[4] - s[0] + s[5] - s[1] + s[6] - s[2] + s[7] - s[3];
  const float gy = s[2] - s[0] + s[3] - s[1] + s[6] - s[4] + s[7] - s[5];
  const float gz = s[1] - s[0] + s[3] - s[2] + s[5] - s[4] + s[7] - s[6];
  const float den = sqrtf(gx * gx + gy * gy + gz * gz) + 1.0e-8f;
  const float half_s = 0.5f * (float)S;
  const float sc = sd_unhalf(sd_half(shape_scale));     // numpy multiplies the fp16 array by the scalar in fp16
#pragma unroll
  for (int c = 0; c < 3; ++c)       // the product of two fp16 values is exact in fp32: one rounding
    points[slot * 3 + c] = sd_half(sd_unhalf(sd_half(p[c] / half_s - 1.f)) * sc);
  grad[slot * 3 + 0] = sd_half(gx / den);
  grad[slot * 3 + 1] = sd_half(gy / den);
  grad[slot * 3 + 2] = sd_half(gz / den);
  val[slot] = sd_half(v);
}

__global__ __launch_bounds__(SD_T) void sd_occu_kernel(const float* __restrict__ sdf, int S, int64_t n, uint64_t seed,
                                                       int64_t shape, const double* __restrict__ u, float shape_scale,
                                                       uint16_t* __restrict__ points, uint8_t* __restrict__ bits) {
  const int64_t g = (int64_t)blockIdx.x * SD_T + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool neg = false;
  if (g < n) {
    const double factor = (double)(S - 1) / (double)S, top = (double)(S - 1), out_scale = 2.0 * (double)shape_scale;
    double q[3];
    bool inside = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double uc;
      if (u) uc = u[g * 3 + c];
      else uc = (double)(mt_step(mt_step(mt_step(seed, (uint64_t)shape), (uint64_t)g), (uint64_t)c) >> 11) * 0x1p-53;
      const double pu = uc * factor;
      points[g * 3 + c] = sd_half((pu - 0.5) * out_scale);
      q[c] = pu * (double)S;
      inside = inside && q[c] >= 0.0 && q[c] < top;     // always, for u in [0, 1): keeps a bad `u` inside the lattice
    }
    if (inside) {
      int xi[3];
      double f0[3], f1[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double fl = floor(q[c]);
        xi[c] = (int)fl;
        f0[c] = fabs(q[c] - fl);
        f1[c] = fabs(q[c] - (fl + 1.0));
      }
      double t[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const double wx = 1.0 - ((c & 4) ? f1[0] : f0[0]);
        const double wy = 1.0 - ((c & 2) ? f1[1] : f0[1]);
        const double wz = 1.0 - ((c & 1) ? f1[2] : f0[2]);
        const float sv = sdf[((int64_t)(xi[0] + (c >> 2)) * S + (xi[1] + ((c >> 1) & 1))) * S + xi[2] + (c & 1)];
        t[c] = (double)sv * ((wx * wy) * wz);
      }
      neg = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7])) < 0.0;
    }
  }
  const uint64_t m = __ballot(neg);                      // lanes past n vote 0: the last byte is zero-padded
  if ((lane & 7) == 0 && g < n) bits[g >> 3] = (uint8_t)(__brev((uint32_t)(m >> lane) & 0xffu) >> 24);
}

inline size_t sd_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct SdWs {
  int32_t* cnt;     // [blocks]      kept samples per block
  int32_t* pre;     // [blocks + 1]  exclusive scan of cnt
  void* scan_ws;
};

size_t sd_layout(int64_t blocks, char* base, SdWs* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += sd_align(bytes);
    return p;
  };
  SdWs l;
  l.cnt = (int32_t*)take(blocks * sizeof(int32_t));
  l.pre = (int32_t*)take((blocks + 1) * sizeof(int32_t));
  l.scan_ws = take(ofx_scan_ws_bytes(blocks));
  if (w) *w = l;
  return off;
}

bool sd_valid(int64_t n_nodes, int k) { return n_nodes >= 0 && k >= 1 && n_nodes <= (INT32_MAX - SD_T) / k; }

}  // namespace

extern "C" size_t ofx_sdf_sample_ws_bytes(int64_t n_nodes, int k) {
  if (!sd_valid(n_nodes, k) || n_nodes == 0) return 0;
  return sd_layout(ofx_cdiv(n_nodes * k, SD_T), nullptr, nullptr);
}

extern "C" int ofx_sdf_sample_nodes(const float* sdf, int S, const int32_t* xyz, int64_t n_nodes,
                                    const int64_t* depth_off, int n_depths, int depth_start, int k, uint64_t seed,
                                    int64_t shape, const float* u, float shape_scale, void* ws, uint16_t* points,
                                    uint16_t* grad, uint16_t* out_sdf, int64_t* count, void* stream) {
  if (!sdf || !count || S < 2 || k < 1 || n_depths < 1 || depth_start < 0 || depth_start + n_depths > 31 ||
      !sd_valid(n_nodes, k))
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  if (n_nodes == 0) {
    if (hipMemsetAsync(count, 0, sizeof(int64_t), st) != hipSuccess) return OFX_ELAUNCH;
    return OFX_OK;
  }
  if (!xyz || !depth_off || !ws || !points || !grad || !out_sdf) return OFX_EINVAL;
  SdNodes a{sdf, xyz, depth_off, u, n_nodes * k, S, n_depths, depth_start, k, seed, shape};
  const int64_t blocks = ofx_cdiv(a.total, SD_T);
  SdWs w;
  sd_layout(blocks, (char*)ws, &w);
  sd_count_kernel<<<(unsigned)blocks, SD_T, 0, st>>>(a, w.cnt);
  OFX_LAUNCH_CHECK();
  const int rc = ofx_scan_i32(w.cnt, w.pre, blocks, w.scan_ws, stream);
  if (rc) return rc;
  sd_emit_kernel<<<(unsigned)blocks, SD_T, 0, st>>>(a, w.pre, shape_scale, points, grad, out_sdf, count);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" int ofx_sdf_sample_occu(const float* sdf, int S, int64_t n, uint64_t seed, int64_t shape, const double* u,
                                   float shape_scale, uint16_t* points, uint8_t* bits, void* stream) {
  if (!sdf || S < 2 || n < 0 || ofx_cdiv(n, SD_T) > INT32_MAX) return OFX_EINVAL;
  if (n == 0) return OFX_OK;
  if (!points || !bits) return OFX_EINVAL;
  sd_occu_kernel<<<(unsigned)ofx_cdiv(n, SD_T), SD_T, 0, ofx_stream(stream)>>>(sdf, S, n, seed, shape, u, shape_scale,
                                                                             points, bits);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

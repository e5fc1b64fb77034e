// The device-side octree view and the NeuralMPU point evaluation, shared by the sweep kernels of ofx_graph.hip
// (ofx_mpu_eval / ofx_mpu_eval_grid) and the brick mesher of ofx_fieldmesh.hip: both must give the same bits for the
// same lattice point, so there is exactly one copy of the arithmetic.
#pragma once
#include "ofx_common.h"

struct TreeDev {
  int depth, full_depth, batch_size;
  const int32_t* child;
  const int64_t* key;
  const int32_t* leafrank;
  int64_t ncum[OFX_MAX_DEPTH + 2];
  int64_t nnum[OFX_MAX_DEPTH + 1];
  int64_t leaf_base[OFX_MAX_DEPTH + 2];  // leaf_base[t] = sum_{s=fd}^{t-1} lnum[s]
};

static int make_tree(const ofx_tree_t* t, TreeDev& T) {
  if (!t || t->depth < 0 || t->depth > OFX_MAX_DEPTH || t->full_depth < 0 || t->full_depth > t->depth ||
      t->batch_size < 1 || !t->child_all || !t->key_all || !t->nnum_host || !t->nnum_nempty_host)
    return OFX_EINVAL;
  T.depth = t->depth;
  T.full_depth = t->full_depth;
  T.batch_size = t->batch_size;
  T.child = t->child_all;
  T.key = t->key_all;
  T.leafrank = t->leafrank_all;
  int64_t c = 0, lb = 0;
  for (int d = 0; d <= OFX_MAX_DEPTH; ++d) {
    T.ncum[d] = c;
    T.leaf_base[d] = lb;
    if (d <= t->depth) {
      T.nnum[d] = t->nnum_host[d];
      c += t->nnum_host[d];
      if (d >= t->full_depth) lb += t->nnum_host[d] - t->nnum_nempty_host[d];
    } else {
      T.nnum[d] = 0;
    }
  }
  T.ncum[OFX_MAX_DEPTH + 1] = c;
  T.leaf_base[OFX_MAX_DEPTH + 1] = lb;
  return OFX_OK;
}

// Index inside depth d of the node of cell (x, y, z) of shape b, or -1 if the octree has no such node.
__device__ __forceinline__ int64_t mpu_walk(const TreeDev& T, int d, int x, int y, int z, int b) {
  const int fd = T.full_depth < d ? T.full_depth : d;
  int sh = d - fd;
  int64_t idx = ((int64_t)b << (3 * fd)) + (int64_t)ofx_xyz2morton(x >> sh, y >> sh, z >> sh);
  for (int s = fd; s < d; ++s) {
    const int32_t c = T.child[T.ncum[s] + idx];
    if (c < 0) return -1;
    sh = d - s - 1;
    idx = (int64_t)c * 8 + ((((x >> sh) & 1) << 2) | (((y >> sh) & 1) << 1) | ((z >> sh) & 1));
  }
  return idx;
}

// Lattice coordinates of the sweep: samples = mgrid * ((bbmax - bbmin) / size) + bbmin in fp32, two roundings
// (util_dualoctree.py:102-103).
__device__ __forceinline__ void mpu_lattice_point(int ix, int iy, int iz, float step, float bbmin, float& px, float& py,
                                                  float& pz) {
  float mx = (float)ix * step, my = (float)iy * step, mz = (float)iz * step;
  asm volatile("" : "+v"(mx), "+v"(my), "+v"(mz));            // keep the product rounded: no fma contraction
  px = mx + bbmin; py = my + bbmin; pz = mz + bbmin;
}

// NeuralMPU value at (px, py, pz) of shape b.  Eight consecutive lanes of a wave (lane & ~7 .. lane | 7) evaluate one
// point, one surrounding cell centre each, and ALL eight get the result; every lane of the wave must call it (the
// parent lookups and the sums go through cross-lane moves).  found_last: this lane's centre exists at depth de.
__device__ __forceinline__ float mpu_eval_point(const TreeDev& T, int ds, int de, const float* __restrict__ code,
                                                float px, float py, float pz, int b, int lane, bool& found_last) {
  const int corner = lane & 7;
  const int dx = (corner >> 2) & 1, dy = (corner >> 1) & 1, dz = corner & 1;      // mpu.py:37-52
  const int lane_base = lane & ~7;
  float num = 0.f, den = 0.f;
  found_last = false;
  int64_t base_rows = 0;
  int prev_idx = -1;
  int pbx = 0, pby = 0, pbz = 0;
  const bool bok = b >= 0 && b < T.batch_size;
  for (int d = ds; d <= de; ++d) {
    const int scale = 1 << d;
    const float half = 0.5f * (float)scale;
    // (p + 1) * scale/2 - 0.5: the product is exact (power of two), so contraction cannot change it
    const float x = (px + 1.0f) * half - 0.5f, y = (py + 1.0f) * half - 0.5f, z = (pz + 1.0f) * half - 0.5f;
    const float bxf = floorf(x), byf = floorf(y), bzf = floorf(z);
    const int bx = (int)bxf, by = (int)byf, bz = (int)bzf;
    const int cx = bx + dx, cy = by + dy, cz = bz + dz;
    const float fx = x - (bxf + (float)dx), fy = y - (byf + (float)dy), fz = z - (bzf + (float)dz);
    const bool inb = bok && cx >= 0 && cy >= 0 && cz >= 0 && cx < scale && cy < scale && cz < scale;
    int idx = -1;
    if (d == ds) {
      if (inb) idx = (int)mpu_walk(T, d, cx, cy, cz, b);
    } else {
      const int pcx = (cx >> 1) - pbx, pcy = (cy >> 1) - pby, pcz = (cz >> 1) - pbz;
      const bool pc_ok = (unsigned)pcx < 2u && (unsigned)pcy < 2u && (unsigned)pcz < 2u;
      const int sl = (inb && pc_ok) ? ((pcx << 2) | (pcy << 1) | pcz) : 0;
      const int pidx = __shfl(prev_idx, lane_base + sl);           // every lane takes part
      if (inb && pc_ok) {
        if (pidx >= 0) {
          const int32_t c = T.child[T.ncum[d - 1] + pidx];
          if (c >= 0) idx = c * 8 + (((cx & 1) << 2) | ((cy & 1) << 1) | (cz & 1));
        }
      } else if (inb) {
        idx = (int)mpu_walk(T, d, cx, cy, cz, b);                  // not reachable in exact arithmetic; kept for safety
      }
    }
    const bool found = idx >= 0;
    if (d == de) found_last = found;
    bool use = found;
    if (found && d < de) use = T.child[T.ncum[d] + idx] < 0;                      // leaves only (mpu.py:113-116)
    if (use) {
      const float4 c = reinterpret_cast<const float4*>(code)[base_rows + idx];
      const float s = 2.0f / (float)scale;
      const float val = c.x * (fx * s) + c.y * (fy * s) + c.z * (fz * s) + c.w;
      const float w = ((1.0f - fabsf(fx)) * (1.0f - fabsf(fy))) * (1.0f - fabsf(fz)) * (float)((double)(d * d) / 50.0);
      num += w * val;
      den += w;
    }
    prev_idx = idx;
    pbx = bx; pby = by; pbz = bz;
    base_rows += T.nnum[d];
  }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) {
    num += __shfl_xor(num, o);
    den += __shfl_xor(den, o);
  }
  return num / (den + 1e-8f);
}

// Voxel meshes of generated octrees (the reference's export_octree, models/octfusion_model_union.py:403-422, which
// scatters the nodes into a dense float grid and runs voxel2mesh, ldm_diffusion_util.py:345-446, a Python loop over
// the occupied voxels): one quad for every cube face whose neighbour is empty.
//
// Contract (include/ofx.h; restated by tests/voxmesh_oracle.py).  R = 2^depth.  Occupancy is a bitmask per shape:
// cell (x, y, z) is bit (x*R + y)*R + z of the shape's ceil(R^3 / 64) uint64 words, x slowest -- ascending bit order
// is the reference's emission order (np.where).  Faces of a cell in the order +z, -z, -x, +x, +y, -y; a face is exposed
// when the neighbour bit is clear or the cell lies on the grid boundary (the reference pads with zeros).  Order comes
// from popcounts and scans, never from atomics: the output is bitwise reproducible.  The only atomics are the
// order-independent atomicOr of the two bitmasks.  Limits: 1 <= depth <= 9, 1 <= batch <= 65535 (the second grid
// dimension of the dense fill) and batch * R^3 * 24 <= INT32_MAX; ofx_voxmesh_ws_bytes returns 0 and the entries
// OFX_EINVAL outside.
//
// Passes.
//   fill   (ofx_voxmesh_mask_keys / _mask_dense): octree keys are decoded and set with atomicOr on a cleared mask;
//          a dense grid is one ballot per 64 cells.
//   count  (ofx_voxmesh_count): one thread per mask word builds the six exposure words -- the neighbour words are
//          funnel shifts by 1, R, R^2 bits over two adjacent words, the grid boundary is a mask per direction -- and
//          sums their popcounts; ofx_scan_i32 over the words of the whole batch.  Welded: one wave per word with a face
//          (a lane per cell) ORs the corners of its exposed faces into a second bitmask over the (R+1)^3 lattice
//          corners, whose per-word popcounts are scanned too.  A finishing kernel writes the per-shape counts.
//   emit   (ofx_voxmesh_emit): one wave per mask word with a face, a lane per cell: the rank of a face is the word's
//          scanned prefix plus the popcounts of the exposure words below the lane.  Unwelded: four vertices per face.
//          Welded: a corner's id is the scanned prefix of its corner-mask word plus the popcount of the lower bits;
//          a lane per corner bit writes the vertices.
#include "ofx_common.h"

#include <cmath>

namespace {

constexpr int VM_T = 256;          // threads per block (4 waves)
constexpr int VM_MAX_DEPTH = 9;
constexpr int VM_BOUND = 24;       // batch * R^3 * 24 <= INT32_MAX: 6 quads = 12 triangles = 24 unwelded vertices a cell
constexpr int VM_MAX_BATCH = 65535;  // the dense fill puts the shape into the grid's y dimension

// Faces in emission order +z, -z, -x, +x, +y, -y.  VM_QUAD: the four corners of the face, 4 bits each, corner code
// dx*4 + dy*2 + dz, first corner in the low bits.  VM_TRI: two triangles, six 2-bit indices into those four corners.
// VM_SIDE: the set of corner codes on the face.
constexpr uint32_t VM_QUAD[6] = {0x3751, 0x2640, 0x3210, 0x7654, 0x7362, 0x5140};
#define VM_TRI6(a, b, c, d, e, f) ((a) | ((b) << 2) | ((c) << 4) | ((d) << 6) | ((e) << 8) | ((f) << 10))
constexpr uint32_t VM_TRI[6] = {VM_TRI6(0, 1, 3, 1, 2, 3), VM_TRI6(1, 0, 3, 2, 1, 3), VM_TRI6(0, 1, 3, 2, 0, 3),
                                VM_TRI6(1, 0, 3, 0, 2, 3), VM_TRI6(1, 0, 3, 0, 2, 3), VM_TRI6(0, 1, 3, 2, 0, 3)};
constexpr uint32_t VM_SIDE[6] = {0xAA, 0x55, 0x0F, 0xF0, 0xCC, 0x33};

struct VmWs {
  uint64_t* mask;   // [B][nW]       occupancy
  int32_t* cnt;     // [B*nW]        faces per mask word
  int32_t* pre;     // [B*nW + 1]    exclusive scan of cnt
  uint32_t* cmask;  // [B][nCW]      welded: used lattice corners
  int32_t* ccnt;    // [B*nCW]       popcounts of cmask
  int32_t* cpre;    // [B*nCW + 1]   exclusive scan of ccnt
  void* scan_ws;    // ofx_scan_i32 workspace for max(B*nW, B*nCW)
};

inline size_t vm_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline int64_t vm_cells(int depth) { return (int64_t)1 << (3 * depth); }
inline int64_t vm_nw(int depth) { return ofx_cdiv(vm_cells(depth), 64); }
inline int64_t vm_ncw(int depth) {
  const int64_t r1 = ((int64_t)1 << depth) + 1;
  return ofx_cdiv(r1 * r1 * r1, 32);
}

bool vm_valid(int batch, int depth) {
  return batch >= 1 && batch <= VM_MAX_BATCH && depth >= 1 && depth <= VM_MAX_DEPTH &&
         (int64_t)batch * vm_cells(depth) * VM_BOUND <= INT32_MAX;
}

size_t vm_layout(int batch, int depth, bool weld, char* base, VmWs* w) {
  const int64_t n1 = (int64_t)batch * vm_nw(depth), n2 = weld ? (int64_t)batch * vm_ncw(depth) : 0;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += vm_align(bytes);
    return p;
  };
  VmWs l;
  l.mask = (uint64_t*)take(n1 * sizeof(uint64_t));     // first: the fill calls do not know `weld`
  l.cnt = (int32_t*)take(n1 * sizeof(int32_t));
  l.pre = (int32_t*)take((n1 + 1) * sizeof(int32_t));
  l.scan_ws = take(ofx_scan_ws_bytes(n1 > n2 ? n1 : n2));
  l.cmask = (uint32_t*)take(n2 * sizeof(uint32_t));
  l.ccnt = (int32_t*)take(n2 * sizeof(int32_t));
  l.cpre = (int32_t*)take((n2 + 1) * sizeof(int32_t));
  if (w) *w = l;
  return off;
}

// ---- fill ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VM_T) void vm_keys_kernel(const int64_t* __restrict__ keys, int64_t n, int batch0,
                                                       int batch, int depth, int64_t nW, uint32_t* __restrict__ mask32) {
  const int64_t i = (int64_t)blockIdx.x * VM_T + threadIdx.x;
  if (i >= n) return;
  int x, y, z, b;
  ofx_key2xyz(keys[i], x, y, z, b);
  const int R = 1 << depth;
  b -= batch0;
  if (b < 0 || b >= batch || x >= R || y >= R || z >= R) return;   // not of this group / not a key of this depth
  const uint32_t idx = (((uint32_t)x << depth) | (uint32_t)y) << depth | (uint32_t)z;
  atomicOr(mask32 + ((int64_t)b * nW * 2 + (idx >> 5)), 1u << (idx & 31));   // little endian: bit idx of the uint64 words
}

__global__ __launch_bounds__(VM_T) void vm_dense_kernel(const float* __restrict__ occ, int64_t n3, int64_t nW,
                                                        float threshold, uint64_t* __restrict__ mask) {
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * VM_T + threadIdx.x;   // cell; a wave covers one mask word
  const int64_t w = i >> 6;
  if (w >= nW) return;                                          // uniform over the wave
  bool on = false;
  if (i < n3) {                                                 // R^3 < 64: the word's upper bits stay clear
    const float v = occ[(int64_t)b * n3 + i];
    on = v > threshold && isfinite(v);
  }
  const uint64_t m = __ballot(on);
  if ((threadIdx.x & 63) == 0) mask[(int64_t)b * nW + w] = m;
}

// ---- exposure --------------------------------------------------------------------------------------------------------
// Bits i of a word whose cell index base + i has the depth-bit field at bit `sh` equal to `target`.
__device__ __forceinline__ uint64_t vm_field_eq(uint32_t base, int sh, int depth, uint32_t target) {
  const uint64_t LANE[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
                            0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
  uint64_t m = ~0ull;
#pragma unroll
  for (int k = 0; k < VM_MAX_DEPTH; ++k) {
    if (k >= depth) break;
    const int bit = sh + k;
    const uint32_t want = (target >> k) & 1u;
    if (bit < 6) {
      uint64_t lane = 0;
#pragma unroll
      for (int q = 0; q < 6; ++q) lane = bit == q ? LANE[q] : lane;
      m &= want ? lane : ~lane;
    } else if (((base >> bit) & 1u) != want) {
      m = 0;
    }
  }
  return m;
}

__device__ __forceinline__ uint64_t vm_word(const uint64_t* __restrict__ m, int64_t w, int64_t nW) {
  return w >= 0 && w < nW ? m[w] : 0ull;
}

// The word whose bit i is the occupancy of cell (64 w + i) + off resp. - off; zero outside the shape.
__device__ __forceinline__ uint64_t vm_up(const uint64_t* __restrict__ m, int64_t w, int64_t nW, int off) {
  const int ws = off >> 6, bs = off & 63;
  const uint64_t lo = vm_word(m, w + ws, nW);
  if (bs == 0) return lo;
  return (lo >> bs) | (vm_word(m, w + ws + 1, nW) << (64 - bs));
}
__device__ __forceinline__ uint64_t vm_down(const uint64_t* __restrict__ m, int64_t w, int64_t nW, int off) {
  const int ws = off >> 6, bs = off & 63;
  const uint64_t hi = vm_word(m, w - ws, nW);
  if (bs == 0) return hi;
  return (hi << bs) | (vm_word(m, w - ws - 1, nW) >> (64 - bs));
}

// The six exposure words of word w of one shape's mask `m`, in emission order.
__device__ __forceinline__ void vm_exposure(const uint64_t* __restrict__ m, int64_t w, int64_t nW, int depth,
                                            uint64_t (&E)[6]) {
  const uint64_t cur = m[w];
  if (cur == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) E[k] = 0;
    return;
  }
  const uint32_t base = (uint32_t)(w << 6), top = (1u << depth) - 1u;
  const int R = 1 << depth, RR = 1 << (2 * depth);
  E[0] = cur & (~vm_up(m, w, nW, 1) | vm_field_eq(base, 0, depth, top));             // +z
  E[1] = cur & (~vm_down(m, w, nW, 1) | vm_field_eq(base, 0, depth, 0));             // -z
  E[2] = cur & (~vm_down(m, w, nW, RR) | vm_field_eq(base, 2 * depth, depth, 0));    // -x
  E[3] = cur & (~vm_up(m, w, nW, RR) | vm_field_eq(base, 2 * depth, depth, top));    // +x
  E[4] = cur & (~vm_up(m, w, nW, R) | vm_field_eq(base, depth, depth, top));         // +y
  E[5] = cur & (~vm_down(m, w, nW, R) | vm_field_eq(base, depth, depth, 0));         // -y
}

// ---- count -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VM_T) void vm_count_kernel(const uint64_t* __restrict__ mask, int64_t nW, int64_t n,
                                                        int depth, int32_t* __restrict__ cnt) {
  const int64_t g = (int64_t)blockIdx.x * VM_T + threadIdx.x;
  if (g >= n) return;
  const int64_t b = g / nW, w = g - b * nW;
  uint64_t E[6];
  vm_exposure(mask + b * nW, w, nW, depth, E);
  int c = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) c += __popcll(E[k]);
  cnt[g] = c;
}

// One wave per mask word, a lane per cell: OR the corners of the exposed faces into the corner mask.
__global__ __launch_bounds__(VM_T) void vm_mark_kernel(const uint64_t* __restrict__ mask, int64_t nW, int64_t n,
                                                       int depth, const int32_t* __restrict__ cnt, int64_t nCW,
                                                       uint32_t* __restrict__ cmask) {
  const int64_t g = ((int64_t)blockIdx.x * VM_T + threadIdx.x) >> 6;
  if (g >= n || cnt[g] == 0) return;                              // uniform over the wave
  const int lane = threadIdx.x & 63;
  const int64_t b = g / nW, w = g - b * nW;
  uint64_t E[6];
  vm_exposure(mask + b * nW, w, nW, depth, E);
  uint32_t used = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) used |= ((E[k] >> lane) & 1ull) ? VM_SIDE[k] : 0u;
  if (!used) return;
  const uint32_t idx = (uint32_t)(w << 6) + lane, top = (1u << depth) - 1u, R1 = top + 2u;
  const uint32_t x = idx >> (2 * depth), y = (idx >> depth) & top, z = idx & top;
  uint32_t* cm = cmask + b * nCW;
#pragma unroll
  for (int code = 0; code < 8; ++code) {
    if (!((used >> code) & 1u)) continue;
    const uint32_t c = ((x + (code >> 2)) * R1 + y + ((code >> 1) & 1)) * R1 + z + (code & 1);
    atomicOr(cm + (c >> 5), 1u << (c & 31));
  }
}

__global__ __launch_bounds__(VM_T) void vm_cpop_kernel(const uint32_t* __restrict__ cmask, int64_t n,
                                                       int32_t* __restrict__ ccnt) {
  const int64_t i = (int64_t)blockIdx.x * VM_T + threadIdx.x;
  if (i < n) ccnt[i] = __popc(cmask[i]);
}

__global__ void vm_counts_kernel(const int32_t* __restrict__ pre, int64_t nW, const int32_t* __restrict__ cpre,
                                 int64_t nCW, int batch, int64_t* __restrict__ counts) {
  for (int b = threadIdx.x; b < batch; b += blockDim.x) {
    counts[2 * b] = (int64_t)pre[(int64_t)(b + 1) * nW] - pre[(int64_t)b * nW];
    counts[2 * b + 1] = cpre ? (int64_t)cpre[(int64_t)(b + 1) * nCW] - cpre[(int64_t)b * nCW] : 0;
  }
}

// ---- emit ------------------------------------------------------------------------------------------------------------
template <bool WELD>
__global__ __launch_bounds__(VM_T) void vm_face_kernel(const uint64_t* __restrict__ mask, int64_t nW, int64_t n,
                                                       int depth, const int32_t* __restrict__ pre, int64_t nCW,
                                                       const uint32_t* __restrict__ cmask,
                                                       const int32_t* __restrict__ cpre,
                                                       const int64_t* __restrict__ vert_off,
                                                       const int64_t* __restrict__ tri_off, float* __restrict__ verts,
                                                       int32_t* __restrict__ faces) {
  const int64_t g = ((int64_t)blockIdx.x * VM_T + threadIdx.x) >> 6;
  if (g >= n) return;
  const int32_t first = pre[g];
  if (pre[g + 1] == first) return;                                // no face in this word (uniform over the wave)
  const int lane = threadIdx.x & 63;
  const int64_t b = g / nW, w = g - b * nW;
  uint64_t E[6];
  vm_exposure(mask + b * nW, w, nW, depth, E);
  const uint64_t below = (1ull << lane) - 1ull;
  int q = first - pre[b * nW];                                    // shape-relative rank of this cell's first face
  uint32_t f = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    q += __popcll(E[k] & below);
    f |= (uint32_t)((E[k] >> lane) & 1ull) << k;
  }
  if (!f) return;
  const uint32_t idx = (uint32_t)(w << 6) + lane, top = (1u << depth) - 1u, R1 = top + 2u;
  const uint32_t x = idx >> (2 * depth), y = (idx >> depth) & top, z = idx & top;
  const float step = 2.0f / (float)(1 << depth);                  // corner * step - 1 is exact in fp32
  const uint32_t* cm = WELD ? cmask + b * nCW : nullptr;
  const int32_t* cp = WELD ? cpre + b * nCW : nullptr;
  float* vout = verts + vert_off[b] * 3;
  int32_t* fout = faces + tri_off[b] * 3;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    if (!((f >> k) & 1u)) continue;
    int vid[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t code = (VM_QUAD[k] >> (4 * j)) & 7u;
      const uint32_t cx = x + (code >> 2), cy = y + ((code >> 1) & 1u), cz = z + (code & 1u);
      if (WELD) {
        const uint32_t c = (cx * R1 + cy) * R1 + cz;
        vid[j] = cp[c >> 5] - cp[0] + __popc(cm[c >> 5] & ((1u << (c & 31)) - 1u));
      } else {
        vid[j] = 4 * q + j;
        float* o = vout + (int64_t)vid[j] * 3;
        o[0] = __fsub_rn(__fmul_rn((float)cx, step), 1.0f);
        o[1] = __fsub_rn(__fmul_rn((float)cy, step), 1.0f);
        o[2] = __fsub_rn(__fmul_rn((float)cz, step), 1.0f);
      }
    }
    int32_t* o = fout + (int64_t)q * 6;
#pragma unroll
    for (int e = 0; e < 6; ++e) o[e] = vid[(VM_TRI[k] >> (2 * e)) & 3u];
    ++q;
  }
}

// Welded vertices: a lane per corner-mask bit.
__global__ __launch_bounds__(VM_T) void vm_corner_kernel(const uint32_t* __restrict__ cmask, int64_t nCW, int64_t n,
                                                         int depth, const int32_t* __restrict__ cpre,
                                                         const int64_t* __restrict__ vert_off,
                                                         float* __restrict__ verts) {
  const int64_t t = (int64_t)blockIdx.x * VM_T + threadIdx.x;
  const int64_t g = t >> 5;
  if (g >= n) return;
  const uint32_t bit = (uint32_t)t & 31u, word = cmask[g];
  if (!((word >> bit) & 1u)) return;
  const int64_t b = g / nCW, cw = g - b * nCW;
  const uint32_t c = (uint32_t)(cw << 5) + bit, R1 = (1u << depth) + 1u;
  const uint32_t cz = c % R1, cy = (c / R1) % R1, cx = c / (R1 * R1);
  const int id = cpre[g] - cpre[b * nCW] + __popc(word & ((1u << bit) - 1u));
  const float step = 2.0f / (float)(1 << depth);
  float* o = verts + (vert_off[b] + id) * 3;
  o[0] = __fsub_rn(__fmul_rn((float)cx, step), 1.0f);
  o[1] = __fsub_rn(__fmul_rn((float)cy, step), 1.0f);
  o[2] = __fsub_rn(__fmul_rn((float)cz, step), 1.0f);
}

inline unsigned vm_blocks(int64_t threads) { return (unsigned)ofx_cdiv(threads, VM_T); }

}  // namespace

extern "C" size_t ofx_voxmesh_ws_bytes(int batch, int depth, int weld) {
  if (!vm_valid(batch, depth)) return 0;
  return vm_layout(batch, depth, weld != 0, nullptr, nullptr);
}

extern "C" int ofx_voxmesh_mask_keys(const int64_t* keys, int64_t n, int batch0, int batch, int depth, void* ws,
                                     void* stream) {
  if (!vm_valid(batch, depth) || n < 0 || (n > 0 && !keys) || batch0 < 0 || !ws) return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  VmWs w;
  vm_layout(batch, depth, false, (char*)ws, &w);
  const int64_t nW = vm_nw(depth);
  if (hipMemsetAsync(w.mask, 0, (size_t)batch * nW * sizeof(uint64_t), st) != hipSuccess) return OFX_ELAUNCH;
  if (n == 0) return OFX_OK;
  vm_keys_kernel<<<vm_blocks(n), VM_T, 0, st>>>(keys, n, batch0, batch, depth, nW, (uint32_t*)w.mask);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" int ofx_voxmesh_mask_dense(const float* occ, int batch, int depth, float threshold, void* ws,
                                      void* stream) {
  if (!vm_valid(batch, depth) || !occ || !ws || threshold != threshold) return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  VmWs w;
  vm_layout(batch, depth, false, (char*)ws, &w);
  const int64_t nW = vm_nw(depth);
  vm_dense_kernel<<<dim3(vm_blocks(nW * 64), batch), VM_T, 0, st>>>(occ, vm_cells(depth), nW, threshold, w.mask);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" int ofx_voxmesh_count(int batch, int depth, int weld, void* ws, int64_t* counts, void* stream) {
  if (!vm_valid(batch, depth) || !ws || !counts) return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  VmWs w;
  vm_layout(batch, depth, weld != 0, (char*)ws, &w);
  const int64_t nW = vm_nw(depth), nCW = vm_ncw(depth), n1 = batch * nW, n2 = batch * nCW;
  vm_count_kernel<<<vm_blocks(n1), VM_T, 0, st>>>(w.mask, nW, n1, depth, w.cnt);
  OFX_LAUNCH_CHECK();
  int rc = ofx_scan_i32(w.cnt, w.pre, n1, w.scan_ws, stream);
  if (rc) return rc;
  if (weld) {
    if (hipMemsetAsync(w.cmask, 0, (size_t)n2 * sizeof(uint32_t), st) != hipSuccess) return OFX_ELAUNCH;
    vm_mark_kernel<<<vm_blocks(n1 * 64), VM_T, 0, st>>>(w.mask, nW, n1, depth, w.cnt, nCW, w.cmask);
    vm_cpop_kernel<<<vm_blocks(n2), VM_T, 0, st>>>(w.cmask, n2, w.ccnt);
    OFX_LAUNCH_CHECK();
    rc = ofx_scan_i32(w.ccnt, w.cpre, n2, w.scan_ws, stream);
    if (rc) return rc;
  }
  vm_counts_kernel<<<1, 64, 0, st>>>(w.pre, nW, weld ? w.cpre : nullptr, nCW, batch, counts);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" int ofx_voxmesh_emit(int batch, int depth, int weld, void* ws, const int64_t* vert_off,
                                const int64_t* tri_off, float* verts, int32_t* faces, void* stream) {
  if (!vm_valid(batch, depth) || !ws || !vert_off || !tri_off || !verts || !faces) return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  VmWs w;
  vm_layout(batch, depth, weld != 0, (char*)ws, &w);
  const int64_t nW = vm_nw(depth), nCW = vm_ncw(depth), n1 = batch * nW, n2 = batch * nCW;
  if (weld) {
    vm_face_kernel<true><<<vm_blocks(n1 * 64), VM_T, 0, st>>>(w.mask, nW, n1, depth, w.pre, nCW, w.cmask, w.cpre,
                                                             vert_off, tri_off, verts, faces);
    vm_corner_kernel<<<vm_blocks(n2 * 32), VM_T, 0, st>>>(w.cmask, nCW, n2, depth, w.cpre, vert_off, verts);
  } else {
    vm_face_kernel<false><<<vm_blocks(n1 * 64), VM_T, 0, st>>>(w.mask, nW, n1, depth, w.pre, 0, nullptr, nullptr,
                                                              vert_off, tri_off, verts, faces);
  }
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

// Connected components of batch meshes and extraction of the largest one (export_mesh's clean=True: the reference
// splits with trimesh and keeps the component whose bounding box has the largest side,
// models/octfusion_model_union.py:459-467; the same code in octfusion_model_vae.py:242-250).
//
// Contract (include/ofx.h; restated by tests/cc_oracle.py).  The mesh is in the layout ofx_mc_emit writes: verts
// [V, 3] fp32, faces [F, 3] int32 local to each shape, vert_off / tri_off int64 [batch + 1].  Two vertices are
// connected when a face uses both; label[v] = the lowest vertex id of v's component within its shape; a vertex no face
// uses is its own label and belongs to no component.  Components with a face are numbered by ascending label.  The
// winner of a shape has the largest max-axis bounding-box extent (fp32 subtraction of the stored coordinates); a tie
// goes to the lowest label.  Kept vertices and faces stay in their order.  Every output is a function of the mesh
// alone: order comes from scans, labels and boxes from integer min / max atomics, never from arrival order.
//
// Passes (global vertex id g = vert_off[b] + v inside the kernels; every pass after `check` returns at once when the
// check found a face index out of range, so a bad index never becomes an address):
//   label   check   F   every index in [0, n_verts of its shape)                            -> status[1]
//           init    V   parent[g] = g
//           hook    F   union(a, b), union(b, c): find with path halving, then CAS the larger root under the smaller
//           flatten V   label[g] = find(g) - vert_off[b]   (a launch of its own; halving goes on)
//   table   flag    F   flag[root of the face] = 1;  scan(flag) -> dense component ids;  comp_of_vert, comp_off
//   stats   V (+F)  bounding boxes by atomicMin / atomicMax on an order-preserving uint32 encoding, exact counts;
//                   a wave whose lanes all belong to one component reduces first and issues one set of atomics
//   select  V       roots only: extent of the component's row -> one packed 64-bit atomicMax per shape on
//                   (extent bits << 32 | ~label);  keep flags;  scan(keep flags of vertices / of faces) -> counts
//   extract V, F    compaction through the two scans, indices renumbered
//
// Visibility (gfx950: eight XCDs with private L2s).  In the hook and flatten launches every read of the parent array
// is a relaxed agent-scope atomic load and every write an agent-scope atomic (CAS, min): a stale parent would only
// cost a retry, but a plain load may be served from a line this CU cached before another XCD's hook.  All other
// arrays are written in one launch and read with plain loads in a later one.  No block ever waits for another: a CAS
// that fails means another hook made progress.  Every loop is capped; a tripped cap sets status[0] (the Python layer
// raises OfxError) and the launch ends.
#include "ofx_common.h"

#include <climits>

namespace {

constexpr int CC_T = 256;
constexpr int CC_FIND_CAP = 1 << 22;   // parent steps of one union / one flatten (halving keeps real chains far below)
constexpr int CC_HOOK_CAP = 1 << 12;   // CAS retries of one union
constexpr int CC_ROW_SEL = 6;          // select's table in the workspace: min[3], max[3]
constexpr int CC_ROW = 8;              // the public table: min[3], max[3], n_verts, n_faces

struct CcWs {
  int32_t* parent;               // [V]    union-find forest (global ids)
  int32_t* flag;                 // [V]    root-with-faces flags, later the vertex keep flags
  int32_t* pre;                  // [V+1]  scan of flag
  void* scan_ws;                 // ofx_scan_i32 workspace for max(V, F)
  unsigned long long* key;       // [batch] packed selection keys
  int32_t* tab;                  // [min(V, F), 6] select's boxes; aliased by the face keep flags and their scan
  int32_t* fflag;                // [F]
  int32_t* fpre;                 // [F+1]
};

inline size_t cc_align(size_t b) { return (b + 255) & ~(size_t)255; }

bool cc_valid(int64_t V, int64_t F, int batch) {
  return batch >= 1 && V >= 1 && F >= 1 && V <= INT32_MAX && F <= INT32_MAX;
}

size_t cc_layout(int64_t V, int64_t F, int batch, char* base, CcWs* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base ? base + off : nullptr;
    off += cc_align(bytes);
    return p;
  };
  CcWs l;
  l.parent = (int32_t*)take((size_t)V * 4);
  l.flag = (int32_t*)take((size_t)V * 4);
  l.pre = (int32_t*)take((size_t)(V + 1) * 4);
  l.scan_ws = take(ofx_scan_ws_bytes(V > F ? V : F));
  l.key = (unsigned long long*)take((size_t)batch * 8);
  const size_t rows = (size_t)(V < F ? V : F) * CC_ROW_SEL * 4;
  const size_t keep = cc_align((size_t)F * 4) + (size_t)(F + 1) * 4;
  char* u = take(rows > keep ? rows : keep);
  l.tab = (int32_t*)u;
  l.fflag = (int32_t*)u;
  l.fpre = (int32_t*)(u ? u + cc_align((size_t)F * 4) : nullptr);
  if (w) *w = l;
  return off;
}

__device__ __forceinline__ int cc_ld(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the shape that owns item i: the largest b with off[b] <= i (empty shapes have equal offsets and own nothing)
__device__ __forceinline__ int cc_shape(const int64_t* __restrict__ off, int batch, int64_t i) {
  int lo = 0, hi = batch;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

// order-preserving uint32 image of an fp32 value (-0 below +0)
__device__ __forceinline__ uint32_t cc_enc(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cc_dec(uint32_t e) {
  return __uint_as_float((e & 0x80000000u) ? (e ^ 0x80000000u) : ~e);
}

// Root of x with path halving.  parent[y] <= y always (a larger root is hooked under a smaller one), so the min keeps
// the forest a forest whatever the interleaving.  steps counts parent loads over the caller's whole operation.
__device__ __forceinline__ int cc_find(int32_t* parent, int x, int& steps) {
  int p = cc_ld(parent + x);
  while (p != x) {
    if (++steps > CC_FIND_CAP) break;
    const int gp = cc_ld(parent + p);
    if (gp != p) __hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = gp;
  }
  return x;
}

__device__ __forceinline__ void cc_union(int32_t* parent, int a, int b, int32_t* status) {
  if (a == b) return;
  int steps = 0;
  for (int it = 0; it < CC_HOOK_CAP; ++it) {
    a = cc_find(parent, a, steps);
    b = cc_find(parent, b, steps);
    if (steps > CC_FIND_CAP) break;
    if (a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    int expect = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expect, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return;
    a = expect;      // hi got a parent meanwhile: go on from there
    b = lo;
  }
  atomicOr(status, 1);
}

#define CC_LOOP(i, n) \
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

__global__ __launch_bounds__(CC_T) void cc_check_kernel(const int32_t* __restrict__ faces,
                                                        const int64_t* __restrict__ vert_off,
                                                        const int64_t* __restrict__ tri_off, int batch, int64_t V,
                                                        int64_t F, int32_t* status) {
  // the offsets themselves: ascending, from 0 to the totals the host sized everything by
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    bool ok = vert_off[0] == 0 && tri_off[0] == 0 && vert_off[batch] == V && tri_off[batch] == F;
    for (int b = 0; b < batch; ++b) ok = ok && vert_off[b] <= vert_off[b + 1] && tri_off[b] <= tri_off[b + 1];
    if (!ok) atomicOr(status + 1, 2);
  }
  CC_LOOP(f, F) {
    const int b = cc_shape(tri_off, batch, f);
    const int64_t nv = vert_off[b + 1] - vert_off[b];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int64_t i = faces[f * 3 + j];
      bad = bad || i < 0 || i >= nv;
    }
    if (bad) atomicOr(status + 1, 1);
  }
}

__global__ __launch_bounds__(CC_T) void cc_init_kernel(int32_t* __restrict__ parent, int64_t V) {
  CC_LOOP(g, V) parent[g] = (int32_t)g;
}

__global__ __launch_bounds__(CC_T) void cc_hook_kernel(const int32_t* __restrict__ faces,
                                                       const int64_t* __restrict__ vert_off,
                                                       const int64_t* __restrict__ tri_off, int batch, int64_t F,
                                                       int32_t* parent, int32_t* status) {
  if (status[1]) return;
  CC_LOOP(f, F) {
    const int b = cc_shape(tri_off, batch, f);
    const int vo = (int)vert_off[b];
    const int a = vo + faces[f * 3], c = vo + faces[f * 3 + 1], d = vo + faces[f * 3 + 2];
    cc_union(parent, a, c, status);
    cc_union(parent, c, d, status);
  }
}

__global__ __launch_bounds__(CC_T) void cc_flatten_kernel(int32_t* parent, const int64_t* __restrict__ vert_off,
                                                          int batch, int64_t V, int32_t* __restrict__ label,
                                                          int32_t* status) {
  if (status[1]) return;
  CC_LOOP(g, V) {
    int steps = 0;
    const int r = cc_find(parent, (int)g, steps);
    if (steps > CC_FIND_CAP) atomicOr(status, 1);
    label[g] = r - (int)vert_off[cc_shape(vert_off, batch, g)];
  }
}

__global__ __launch_bounds__(CC_T) void cc_flag_kernel(const int32_t* __restrict__ faces,
                                                       const int32_t* __restrict__ label,
                                                       const int64_t* __restrict__ vert_off,
                                                       const int64_t* __restrict__ tri_off, int batch, int64_t F,
                                                       int32_t* __restrict__ flag, const int32_t* __restrict__ status) {
  if (status[1]) return;
  CC_LOOP(f, F) {
    const int64_t vo = vert_off[cc_shape(tri_off, batch, f)];
    flag[vo + label[vo + faces[f * 3]]] = 1;     // every writer stores the same value
  }
}

__global__ __launch_bounds__(CC_T) void cc_ids_kernel(const int32_t* __restrict__ label,
                                                      const int32_t* __restrict__ flag,
                                                      const int32_t* __restrict__ pre,
                                                      const int64_t* __restrict__ vert_off, int batch, int64_t V,
                                                      int32_t* __restrict__ comp_of_vert,
                                                      int32_t* __restrict__ comp_off,
                                                      const int32_t* __restrict__ status) {
  if (status[1]) return;
  if (blockIdx.x == 0)
    for (int b = threadIdx.x; b <= batch; b += blockDim.x) comp_off[b] = pre[vert_off[b]];
  if (!comp_of_vert) return;
  CC_LOOP(g, V) {
    const int64_t vo = vert_off[cc_shape(vert_off, batch, g)];
    const int64_t r = vo + label[g];
    comp_of_vert[g] = flag[r] ? pre[r] - pre[vo] : -1;
  }
}

__global__ __launch_bounds__(CC_T) void cc_rows_init_kernel(const int32_t* __restrict__ pre, int64_t V, int64_t rows,
                                                            int stride, int32_t* __restrict__ tab,
                                                            const int32_t* __restrict__ status) {
  if (status[1]) return;
  const int64_t K = pre[V] < rows ? pre[V] : rows;
  CC_LOOP(i, K * stride) {
    const int c = (int)(i % stride);
    tab[i] = c < 3 ? -1 : 0;          // min: all ones; max and the counts: zero
  }
}

__device__ __forceinline__ int cc_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(v, o);
    v = t > v ? t : v;
  }
  return v;
}

// Boxes (and, with stride 8, vertex counts) of the components.  Whole waves stay in the loop so that a wave whose
// lanes all sit in one component -- nearly every wave of the main body -- issues one set of atomics.
__global__ __launch_bounds__(CC_T) void cc_stats_vert_kernel(const float* __restrict__ verts,
                                                             const int32_t* __restrict__ label,
                                                             const int32_t* __restrict__ flag,
                                                             const int32_t* __restrict__ pre,
                                                             const int64_t* __restrict__ vert_off, int batch,
                                                             int64_t V, int64_t rows, int stride,
                                                             int32_t* __restrict__ tab,
                                                             const int32_t* __restrict__ status) {
  if (status[1]) return;
  uint32_t* t = (uint32_t*)tab;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < V; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = base + threadIdx.x;
    int64_t k = -1;
    uint32_t e[3] = {0, 0, 0};
    if (g < V) {
      const int64_t vo = vert_off[cc_shape(vert_off, batch, g)];
      const int64_t r = vo + label[g];
      if (flag[r]) {
        k = pre[r];
        if (k >= rows) k = -1;
      }
      if (k >= 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) e[a] = cc_enc(verts[g * 3 + a]);
      }
    }
    const int kmax = cc_wave_max((int)k);
    if (kmax < 0) continue;
    if (__all(k < 0 || k == kmax)) {
      uint32_t mn[3], mx[3];
      int cnt = k >= 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        mn[a] = k >= 0 ? e[a] : 0xFFFFFFFFu;
        mx[a] = k >= 0 ? e[a] : 0u;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const uint32_t tn = __shfl_xor(mn[a], o), tx = __shfl_xor(mx[a], o);
          mn[a] = tn < mn[a] ? tn : mn[a];
          mx[a] = tx > mx[a] ? tx : mx[a];
        }
        cnt += __shfl_xor(cnt, o);
      }
      if ((threadIdx.x & 63) == 0) {
        uint32_t* row = t + (int64_t)kmax * stride;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          atomicMin(row + a, mn[a]);
          atomicMax(row + 3 + a, mx[a]);
        }
        if (stride == CC_ROW) atomicAdd((int32_t*)row + 6, cnt);
      }
    } else if (k >= 0) {
      uint32_t* row = t + k * stride;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        atomicMin(row + a, e[a]);
        atomicMax(row + 3 + a, e[a]);
      }
      if (stride == CC_ROW) atomicAdd((int32_t*)row + 6, 1);
    }
  }
}

__global__ __launch_bounds__(CC_T) void cc_stats_face_kernel(const int32_t* __restrict__ faces,
                                                             const int32_t* __restrict__ label,
                                                             const int32_t* __restrict__ pre,
                                                             const int64_t* __restrict__ vert_off,
                                                             const int64_t* __restrict__ tri_off, int batch,
                                                             int64_t F, int64_t rows, int32_t* __restrict__ tab,
                                                             const int32_t* __restrict__ status) {
  if (status[1]) return;
  for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < F; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t f = base + threadIdx.x;
    int64_t k = -1;
    if (f < F) {
      const int64_t vo = vert_off[cc_shape(tri_off, batch, f)];
      k = pre[vo + label[vo + faces[f * 3]]];
      if (k >= rows) k = -1;
    }
    const int kmax = cc_wave_max((int)k);
    if (kmax < 0) continue;
    if (__all(k < 0 || k == kmax)) {
      const int cnt = __popcll(__ballot(k >= 0));
      if ((threadIdx.x & 63) == 0) atomicAdd(tab + (int64_t)kmax * CC_ROW + 7, cnt);
    } else if (k >= 0) {
      atomicAdd(tab + k * CC_ROW + 7, 1);
    }
  }
}

__global__ __launch_bounds__(CC_T) void cc_decode_kernel(const int32_t* __restrict__ pre, int64_t V, int64_t rows,
                                                         int32_t* __restrict__ tab,
                                                         const int32_t* __restrict__ status) {
  if (status[1]) return;
  const int64_t K = pre[V] < rows ? pre[V] : rows;
  CC_LOOP(i, K * 6) {
    const int64_t at = (i / 6) * CC_ROW + i % 6;
    tab[at] = (int32_t)__float_as_uint(cc_dec((uint32_t)tab[at]));
  }
}

// The reference's rule, by the roots: one packed key per shape.  A root first looks at the key and skips the atomic
// when it cannot win, so the one address sees few writers.
__global__ __launch_bounds__(CC_T) void cc_select_kernel(const int32_t* __restrict__ label,
                                                         const int32_t* __restrict__ flag,
                                                         const int32_t* __restrict__ pre,
                                                         const int32_t* __restrict__ tab,
                                                         const int64_t* __restrict__ vert_off, int batch, int64_t V,
                                                         int64_t rows, unsigned long long* key,
                                                         const int32_t* __restrict__ status) {
  if (status[1]) return;
  CC_LOOP(g, V) {
    const int b = cc_shape(vert_off, batch, g);
    const int local = (int)(g - vert_off[b]);
    if (label[g] != local || !flag[g]) continue;
    const int64_t k = pre[g];
    if (k >= rows) continue;
    const uint32_t* row = (const uint32_t*)tab + k * CC_ROW_SEL;
    float ext = __fsub_rn(cc_dec(row[3]), cc_dec(row[0]));
#pragma unroll
    for (int a = 1; a < 3; ++a) ext = fmaxf(ext, __fsub_rn(cc_dec(row[3 + a]), cc_dec(row[a])));
    const unsigned long long mine = ((unsigned long long)__float_as_uint(ext) << 32) | (uint32_t)~local;
    if (__hip_atomic_load(key + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine) atomicMax(key + b, mine);
  }
}

// winner labels, the component counts (before the keep scan reuses `pre`) -- one small block.  This kernel and
// cc_counts_kernel write all of keep_counts, and only when status[1] is clear.
__global__ void cc_winner_kernel(const unsigned long long* __restrict__ key, const int32_t* __restrict__ pre,
                                 const int64_t* __restrict__ vert_off, int batch,
                                 int32_t* __restrict__ winner_label, int64_t* __restrict__ keep_counts,
                                 const int32_t* __restrict__ status) {
  if (status[1]) return;
  for (int b = threadIdx.x; b < batch; b += blockDim.x) {
    winner_label[b] = key[b] ? (int32_t)~(uint32_t)key[b] : -1;
    keep_counts[2 * batch + b] = (int64_t)pre[vert_off[b + 1]] - pre[vert_off[b]];
  }
}

__global__ __launch_bounds__(CC_T) void cc_keep_vert_kernel(const int32_t* __restrict__ label,
                                                            const int32_t* __restrict__ winner_label,
                                                            const int64_t* __restrict__ vert_off, int batch,
                                                            int64_t V, int32_t* __restrict__ flag,
                                                            const int32_t* __restrict__ status) {
  if (status[1]) return;
  CC_LOOP(g, V) flag[g] = label[g] == winner_label[cc_shape(vert_off, batch, g)];
}

__global__ __launch_bounds__(CC_T) void cc_keep_face_kernel(const int32_t* __restrict__ faces,
                                                            const int32_t* __restrict__ label,
                                                            const int32_t* __restrict__ winner_label,
                                                            const int64_t* __restrict__ vert_off,
                                                            const int64_t* __restrict__ tri_off, int batch,
                                                            int64_t F, int32_t* __restrict__ fflag,
                                                            const int32_t* __restrict__ status) {
  if (status[1]) return;
  CC_LOOP(f, F) {
    const int b = cc_shape(tri_off, batch, f);
    fflag[f] = label[vert_off[b] + faces[f * 3]] == winner_label[b];
  }
}

__global__ void cc_counts_kernel(const int32_t* __restrict__ pre, const int32_t* __restrict__ fpre,
                                 const int64_t* __restrict__ vert_off, const int64_t* __restrict__ tri_off,
                                 int batch, int64_t* __restrict__ keep_counts, const int32_t* __restrict__ status) {
  if (status[1]) return;
  for (int b = threadIdx.x; b < batch; b += blockDim.x) {
    keep_counts[b] = (int64_t)pre[vert_off[b + 1]] - pre[vert_off[b]];
    keep_counts[batch + b] = (int64_t)fpre[tri_off[b + 1]] - fpre[tri_off[b]];
  }
}

__global__ __launch_bounds__(CC_T) void cc_extract_vert_kernel(const float* __restrict__ verts,
                                                               const int32_t* __restrict__ pre,
                                                               const int64_t* __restrict__ vert_off,
                                                               const int64_t* __restrict__ new_vert_off, int batch,
                                                               int64_t V, float* __restrict__ out,
                                                               const int32_t* __restrict__ status) {
  if (status[1]) return;
  CC_LOOP(g, V) {
    if (pre[g + 1] == pre[g]) continue;
    const int b = cc_shape(vert_off, batch, g);
    const int64_t dst = new_vert_off[b] + (pre[g] - pre[vert_off[b]]);
#pragma unroll
    for (int a = 0; a < 3; ++a) out[dst * 3 + a] = verts[g * 3 + a];
  }
}

__global__ __launch_bounds__(CC_T) void cc_extract_face_kernel(const int32_t* __restrict__ faces,
                                                               const int32_t* __restrict__ pre,
                                                               const int32_t* __restrict__ fpre,
                                                               const int64_t* __restrict__ vert_off,
                                                               const int64_t* __restrict__ tri_off,
                                                               const int64_t* __restrict__ new_tri_off, int batch,
                                                               int64_t F, int32_t* __restrict__ out,
                                                               const int32_t* __restrict__ status) {
  if (status[1]) return;
  CC_LOOP(f, F) {
    if (fpre[f + 1] == fpre[f]) continue;
    const int b = cc_shape(tri_off, batch, f);
    const int64_t vo = vert_off[b];
    const int64_t dst = new_tri_off[b] + (fpre[f] - fpre[tri_off[b]]);
#pragma unroll
    for (int j = 0; j < 3; ++j) out[dst * 3 + j] = pre[vo + faces[f * 3 + j]] - pre[vo];
  }
}

// flag[] and its scan: which roots carry faces, numbered in label order
int cc_flags(const int32_t* faces, const int32_t* label, const int64_t* vert_off, const int64_t* tri_off, int batch,
             int64_t V, int64_t F, const CcWs& w, const int32_t* status, void* stream) {
  hipStream_t st = ofx_stream(stream);
  if (hipMemsetAsync(w.flag, 0, (size_t)V * 4, st) != hipSuccess) return OFX_ELAUNCH;
  cc_flag_kernel<<<ofx_grid(F, CC_T), CC_T, 0, st>>>(faces, label, vert_off, tri_off, batch, F, w.flag, status);
  OFX_LAUNCH_CHECK();
  return ofx_scan_i32(w.flag, w.pre, V, w.scan_ws, stream);
}

int cc_rows(const float* verts, const int32_t* faces, const int32_t* label, const int64_t* vert_off,
            const int64_t* tri_off, int batch, int64_t V, int64_t F, int64_t rows, int stride, int32_t* tab,
            const CcWs& w, const int32_t* status, hipStream_t st) {
  cc_rows_init_kernel<<<ofx_grid(rows * stride, CC_T), CC_T, 0, st>>>(w.pre, V, rows, stride, tab, status);
  cc_stats_vert_kernel<<<ofx_grid(V, CC_T), CC_T, 0, st>>>(verts, label, w.flag, w.pre, vert_off, batch, V, rows,
                                                          stride, tab, status);
  if (stride == CC_ROW) {
    cc_stats_face_kernel<<<ofx_grid(F, CC_T), CC_T, 0, st>>>(faces, label, w.pre, vert_off, tri_off, batch, F, rows,
                                                            tab, status);
    cc_decode_kernel<<<ofx_grid(rows * 6, CC_T), CC_T, 0, st>>>(w.pre, V, rows, tab, status);
  }
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

}  // namespace

extern "C" size_t ofx_mesh_cc_ws_bytes(int64_t total_verts, int64_t total_faces, int batch) {
  if (!cc_valid(total_verts, total_faces, batch)) return 0;
  return cc_layout(total_verts, total_faces, batch, nullptr, nullptr);
}

extern "C" int ofx_mesh_cc_label(const int32_t* faces, const int64_t* vert_off, const int64_t* tri_off, int batch,
                                 int64_t total_verts, int64_t total_faces, int32_t* label, void* ws, int32_t* status,
                                 void* stream) {
  const int64_t V = total_verts, F = total_faces;
  if (!cc_valid(V, F, batch) || !faces || !vert_off || !tri_off || !label || !ws || !status) return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  CcWs w;
  cc_layout(V, F, batch, (char*)ws, &w);
  if (hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st) != hipSuccess) return OFX_ELAUNCH;
  cc_check_kernel<<<ofx_grid(F, CC_T), CC_T, 0, st>>>(faces, vert_off, tri_off, batch, V, F, status);
  cc_init_kernel<<<ofx_grid(V, CC_T), CC_T, 0, st>>>(w.parent, V);
  cc_hook_kernel<<<ofx_grid(F, CC_T), CC_T, 0, st>>>(faces, vert_off, tri_off, batch, F, w.parent, status);
  cc_flatten_kernel<<<ofx_grid(V, CC_T), CC_T, 0, st>>>(w.parent, vert_off, batch, V, label, status);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" int ofx_mesh_cc_table(const int32_t* faces, const int32_t* label, const int64_t* vert_off,
                                 const int64_t* tri_off, int batch, int64_t total_verts, int64_t total_faces,
                                 int32_t* comp_of_vert, int32_t* comp_off, void* ws, const int32_t* status,
                                 void* stream) {
  const int64_t V = total_verts, F = total_faces;
  if (!cc_valid(V, F, batch) || !faces || !label || !vert_off || !tri_off || !comp_off || !ws || !status)
    return OFX_EINVAL;
  CcWs w;
  cc_layout(V, F, batch, (char*)ws, &w);
  const int rc = cc_flags(faces, label, vert_off, tri_off, batch, V, F, w, status, stream);
  if (rc) return rc;
  cc_ids_kernel<<<ofx_grid(V, CC_T), CC_T, 0, ofx_stream(stream)>>>(label, w.flag, w.pre, vert_off, batch, V,
                                                                   comp_of_vert, comp_off, status);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" int ofx_mesh_cc_stats(const float* verts, const int32_t* faces, const int32_t* label,
                                 const int64_t* vert_off, const int64_t* tri_off, int batch, int64_t total_verts,
                                 int64_t total_faces, int64_t n_comp, int32_t* table, void* ws, const int32_t* status,
                                 void* stream) {
  const int64_t V = total_verts, F = total_faces;
  if (!cc_valid(V, F, batch) || !verts || !faces || !label || !vert_off || !tri_off || n_comp < 0 || !ws || !status)
    return OFX_EINVAL;
  if (n_comp == 0) return OFX_OK;
  if (!table) return OFX_EINVAL;
  CcWs w;
  cc_layout(V, F, batch, (char*)ws, &w);
  return cc_rows(verts, faces, label, vert_off, tri_off, batch, V, F, n_comp, CC_ROW, table, w, status,
                 ofx_stream(stream));
}

extern "C" int ofx_mesh_cc_select(const float* verts, const int32_t* faces, const int32_t* label,
                                  const int64_t* vert_off, const int64_t* tri_off, int batch, int64_t total_verts,
                                  int64_t total_faces, int32_t* winner_label, int64_t* keep_counts, void* ws,
                                  const int32_t* status, void* stream) {
  const int64_t V = total_verts, F = total_faces;
  if (!cc_valid(V, F, batch) || !verts || !faces || !label || !vert_off || !tri_off || !winner_label ||
      !keep_counts || !ws || !status)
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  CcWs w;
  cc_layout(V, F, batch, (char*)ws, &w);
  int rc = cc_flags(faces, label, vert_off, tri_off, batch, V, F, w, status, stream);
  if (rc) return rc;
  const int64_t rows = V < F ? V : F;
  rc = cc_rows(verts, faces, label, vert_off, tri_off, batch, V, F, rows, CC_ROW_SEL, w.tab, w, status, st);
  if (rc) return rc;
  if (hipMemsetAsync(w.key, 0, (size_t)batch * 8, st) != hipSuccess) return OFX_ELAUNCH;
  cc_select_kernel<<<ofx_grid(V, CC_T), CC_T, 0, st>>>(label, w.flag, w.pre, w.tab, vert_off, batch, V, rows, w.key,
                                                      status);
  cc_winner_kernel<<<1, CC_T, 0, st>>>(w.key, w.pre, vert_off, batch, winner_label, keep_counts, status);
  cc_keep_vert_kernel<<<ofx_grid(V, CC_T), CC_T, 0, st>>>(label, winner_label, vert_off, batch, V, w.flag, status);
  cc_keep_face_kernel<<<ofx_grid(F, CC_T), CC_T, 0, st>>>(faces, label, winner_label, vert_off, tri_off, batch, F,
                                                         w.fflag, status);
  OFX_LAUNCH_CHECK();
  rc = ofx_scan_i32(w.flag, w.pre, V, w.scan_ws, stream);
  if (rc) return rc;
  rc = ofx_scan_i32(w.fflag, w.fpre, F, w.scan_ws, stream);
  if (rc) return rc;
  cc_counts_kernel<<<1, CC_T, 0, st>>>(w.pre, w.fpre, vert_off, tri_off, batch, keep_counts, status);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" int ofx_mesh_cc_extract(const float* verts, const int32_t* faces, const int64_t* vert_off,
                                   const int64_t* tri_off, int batch, int64_t total_verts, int64_t total_faces,
                                   const int64_t* new_vert_off, const int64_t* new_tri_off, float* out_verts,
                                   int32_t* out_faces, void* ws, const int32_t* status, void* stream) {
  const int64_t V = total_verts, F = total_faces;
  if (!cc_valid(V, F, batch) || !verts || !faces || !vert_off || !tri_off || !new_vert_off || !new_tri_off ||
      !out_verts || !out_faces || !ws || !status)
    return OFX_EINVAL;
  hipStream_t st = ofx_stream(stream);
  CcWs w;
  cc_layout(V, F, batch, (char*)ws, &w);
  cc_extract_vert_kernel<<<ofx_grid(V, CC_T), CC_T, 0, st>>>(verts, w.pre, vert_off, new_vert_off, batch, V,
                                                            out_verts, status);
  cc_extract_face_kernel<<<ofx_grid(F, CC_T), CC_T, 0, st>>>(faces, w.pre, w.fpre, vert_off, tri_off, new_tri_off,
                                                            batch, F, out_faces, status);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

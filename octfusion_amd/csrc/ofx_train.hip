// libofx: the optimiser side of a training step as a handful of launches.
//   ofx_adamw_ema_multi: AdamW + EMA over a whole list of tensors (torch.optim.AdamW's update followed by
//                        ldm_diffusion_util.py:38-54), the arithmetic of ofx_optim.h, shared with the per-tensor kernels;
//   ofx_mse_grad:        the diffusion stages' MSE loss and its gradient, the loss left on the device.
// Both are HBM-bound elementwise passes: 16-byte accesses where the pointers allow, plain vector stores only.
#include "ofx_common.h"
#include "ofx_optim.h"

// ---------------------------------------------------------------------------------------------------------------------
// Multi-tensor AdamW + EMA.  The tensor table travels BY VALUE in the kernel arguments, a slab of up to MT_ROWS rows per
// launch (the slab is 3336 bytes of the 4 KB argument block): nothing on the device has to outlive the call, so a host that runs a
// step ahead cannot overwrite a table the device still reads.  Every row is cut into chunks of MT_CHUNK elements; chunk c
// of the slab belongs to the row r with chunk0[r] <= c < chunk0[r + 1].  A block takes chunks blockIdx.x, + gridDim.x,
// ...; the row search runs on blockIdx-derived values only, so it is wave-uniform and the table is read with scalar
// loads.  A chunk starts MT_CHUNK * 4 bytes into its row, so its alignment is the row's.
constexpr int MT_ROWS = 64;
constexpr int MT_CHUNK = 4096;
constexpr int MT_THREADS = 256;
constexpr int MT_MAX_GRID = 2048;          // 256 CUs x 8 blocks: the grid-stride cap of a memory-bound pass

struct MtSlab {
  float* p[MT_ROWS];
  const float* g[MT_ROWS];
  float* m[MT_ROWS];
  float* v[MT_ROWS];
  float* e[MT_ROWS];
  int64_t n[MT_ROWS];
  int32_t chunk0[MT_ROWS + 1];
  int32_t rows;
};
static_assert(sizeof(MtSlab) + 64 <= 4096, "the slab and the scalars must fit the kernel argument block");

struct MtScalars {
  float lr, b1, b2, eps, wd, bc1, bc2, ema_beta;
};

template <bool HAS_G, bool HAS_E>
__device__ __forceinline__ void mt_chunk(const OfxAdamW& a, float beta, float* __restrict__ p,
                                         const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                         float* __restrict__ e, int len) {
  uintptr_t bits = (uintptr_t)p;
  if (HAS_G) bits |= (uintptr_t)g | (uintptr_t)m | (uintptr_t)v;
  if (HAS_E) bits |= (uintptr_t)e;
  const int nvec = (bits & 15) ? 0 : (len >> 2);           // wave-uniform: a misaligned row goes element by element
  for (int q = threadIdx.x; q < nvec; q += MT_THREADS) {
    float4 pv = reinterpret_cast<const float4*>(p)[q];
    float pe[4] = {pv.x, pv.y, pv.z, pv.w};
    if (HAS_G) {
      const float4 gv = reinterpret_cast<const float4*>(g)[q];
      float4 mv = reinterpret_cast<const float4*>(m)[q];
      float4 vv = reinterpret_cast<const float4*>(v)[q];
      const float ge[4] = {gv.x, gv.y, gv.z, gv.w};
      float me[4] = {mv.x, mv.y, mv.z, mv.w};
      float ve[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) pe[k] = ofx_adamw_elem(a, pe[k], ge[k], me[k], ve[k]);
      reinterpret_cast<float4*>(m)[q] = make_float4(me[0], me[1], me[2], me[3]);
      reinterpret_cast<float4*>(v)[q] = make_float4(ve[0], ve[1], ve[2], ve[3]);
      reinterpret_cast<float4*>(p)[q] = make_float4(pe[0], pe[1], pe[2], pe[3]);
    }
    if (HAS_E) {                                              // the fresh parameter comes from the registers
      const float4 ev = reinterpret_cast<const float4*>(e)[q];
      reinterpret_cast<float4*>(e)[q] = make_float4(ofx_ema_elem(ev.x, pe[0], beta), ofx_ema_elem(ev.y, pe[1], beta),
                                                     ofx_ema_elem(ev.z, pe[2], beta), ofx_ema_elem(ev.w, pe[3], beta));
    }
  }
  for (int i = (nvec << 2) + threadIdx.x; i < len; i += MT_THREADS) {      // tail, or the whole misaligned chunk
    float pi = p[i];
    if (HAS_G) {
      float mi = m[i], vi = v[i];
      pi = ofx_adamw_elem(a, pi, g[i], mi, vi);
      m[i] = mi;
      v[i] = vi;
      p[i] = pi;
    }
    if (HAS_E) e[i] = ofx_ema_elem(e[i], pi, beta);
  }
}

__global__ __launch_bounds__(MT_THREADS) void adamw_ema_multi_kernel(const MtSlab s, const MtScalars k) {
  const OfxAdamW a = ofx_adamw_setup(k.lr, k.b1, k.b2, k.eps, k.wd, k.bc1, k.bc2);
  const int total = s.chunk0[s.rows];
  for (int c = blockIdx.x; c < total; c += gridDim.x) {
    int lo = 0, hi = s.rows;                                // largest r with chunk0[r] <= c
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s.chunk0[mid] <= c) lo = mid; else hi = mid;
    }
    const int r = lo;
    const int64_t start = (int64_t)(c - s.chunk0[r]) * MT_CHUNK;
    const int64_t left = s.n[r] - start;
    const int len = left < MT_CHUNK ? (int)left : MT_CHUNK;
    float* p = s.p[r] + start;
    const float* g = s.g[r];
    float* e = s.e[r];
    if (g && e) mt_chunk<true, true>(a, k.ema_beta, p, g + start, s.m[r] + start, s.v[r] + start, e + start, len);
    else if (g) mt_chunk<true, false>(a, k.ema_beta, p, g + start, s.m[r] + start, s.v[r] + start, nullptr, len);
    else mt_chunk<false, true>(a, k.ema_beta, p, nullptr, nullptr, nullptr, e + start, len);
  }
}

extern "C" int ofx_adamw_ema_multi_chunk(void) { return MT_CHUNK; }
extern "C" int ofx_adamw_ema_multi_rows(void) { return MT_ROWS; }

static int mt_launch(const MtSlab& s, const MtScalars& k, hipStream_t st) {
  const int total = s.chunk0[s.rows];
  if (total == 0) return OFX_OK;
  adamw_ema_multi_kernel<<<total < MT_MAX_GRID ? total : MT_MAX_GRID, MT_THREADS, 0, st>>>(s, k);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

extern "C" int ofx_adamw_ema_multi(const OfxAdamRow* rows, int64_t n_rows, float lr, float beta1, float beta2, float eps,
                                   float weight_decay, int step, float ema_beta, void* stream) {
  if (n_rows < 0 || step < 1 || (n_rows > 0 && !rows)) return OFX_EINVAL;
  constexpr int64_t MAX_CHUNKS = (int64_t)1 << 30;         // per slab: chunk0 is int32
  for (int64_t i = 0; i < n_rows; ++i) {                   // every row is checked before anything is launched
    const OfxAdamRow& r = rows[i];
    if (r.n < 0) return OFX_EINVAL;
    if (r.n == 0) continue;
    if (!r.param || (r.grad && (!r.exp_avg || !r.exp_avg_sq))) return OFX_EINVAL;
    if (ofx_cdiv(r.n, MT_CHUNK) > MAX_CHUNKS) return OFX_EINVAL;
  }
  MtScalars k;
  k.lr = lr; k.b1 = beta1; k.b2 = beta2; k.eps = eps; k.wd = weight_decay; k.ema_beta = ema_beta;
  k.bc1 = 1.f - powf(beta1, (float)step);
  k.bc2 = 1.f - powf(beta2, (float)step);
  MtSlab s = {};
  for (int64_t i = 0; i < n_rows; ++i) {
    const OfxAdamRow& r = rows[i];
    if (r.n == 0 || (!r.grad && !r.ema)) continue;         // nothing to do for this row
    const int64_t chunks = ofx_cdiv(r.n, MT_CHUNK);
    if (s.rows == MT_ROWS || s.chunk0[s.rows] + chunks > MAX_CHUNKS) {
      const int rc = mt_launch(s, k, ofx_stream(stream));
      if (rc != OFX_OK) return rc;
      s.rows = 0;
    }
    const int j = s.rows++;
    s.p[j] = r.param; s.g[j] = r.grad; s.m[j] = r.exp_avg; s.v[j] = r.exp_avg_sq; s.e[j] = r.ema; s.n[j] = r.n;
    s.chunk0[j + 1] = s.chunk0[j] + (int32_t)chunks;
  }
  return mt_launch(s, k, ofx_stream(stream));
}

// ---------------------------------------------------------------------------------------------------------------------
// MSE loss and gradient of the diffusion stages: dy = (y - target) * (float)(2 / n) -- the two fp32 operations of torch's
// `diff * (2.0 / diff.numel())` -- and *loss_out = mean((double)diff * diff).  Block b leaves the fp64 sum of its
// elements in partials[b]; a second one-block launch adds the partials in a fixed order.  The grid depends on n alone
// and there are no floating-point atomics, so the loss is the same bits run to run.
constexpr int MSE_THREADS = 256;
constexpr int MSE_PER_BLOCK = 4096;
constexpr int MSE_MAX_GRID = 1024;

static inline int64_t mse_blocks(int64_t n) {
  int64_t b = ofx_cdiv(n, MSE_PER_BLOCK);
  return b < 1 ? 1 : (b > MSE_MAX_GRID ? MSE_MAX_GRID : b);
}

__device__ __forceinline__ double mse_block_sum(double acc, double* red) {
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = MSE_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(MSE_THREADS) void mse_grad_kernel(const float* __restrict__ y, const float* __restrict__ t,
                                                               float* __restrict__ dy, double* __restrict__ partials,
                                                               int64_t n, float s) {
  __shared__ double red[MSE_THREADS];
  const int64_t tid = (int64_t)blockIdx.x * MSE_THREADS + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * MSE_THREADS;
  const bool aligned = (((uintptr_t)y | (uintptr_t)t | (uintptr_t)dy) & 15) == 0;
  const int64_t nvec = aligned ? (n >> 2) : 0;
  double acc = 0.0;
  for (int64_t q = tid; q < nvec; q += stride) {
    const float4 a = reinterpret_cast<const float4*>(y)[q];
    const float4 b = reinterpret_cast<const float4*>(t)[q];
    const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
    reinterpret_cast<float4*>(dy)[q] = make_float4(d0 * s, d1 * s, d2 * s, d3 * s);
    acc += (double)d0 * d0;
    acc += (double)d1 * d1;
    acc += (double)d2 * d2;
    acc += (double)d3 * d3;
  }
  for (int64_t i = (nvec << 2) + tid; i < n; i += stride) {
    const float d = y[i] - t[i];
    dy[i] = d * s;
    acc += (double)d * d;
  }
  const double sum = mse_block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

__global__ __launch_bounds__(MSE_THREADS) void mse_finish_kernel(const double* __restrict__ partials, int blocks,
                                                                 double* __restrict__ loss_out, int64_t n) {
  __shared__ double red[MSE_THREADS];
  double acc = 0.0;
  for (int i = threadIdx.x; i < blocks; i += MSE_THREADS) acc += partials[i];
  const double sum = mse_block_sum(acc, red);
  if (threadIdx.x == 0) *loss_out = sum / (double)n;
}

extern "C" int64_t ofx_mse_grad_partials(int64_t n) { return n > 0 ? mse_blocks(n) : 0; }

extern "C" int ofx_mse_grad(const float* y, const float* target, float* dy, double* partials, double* loss_out,
                            int64_t n, void* stream) {
  if (n < 1 || !y || !target || !dy || !partials || !loss_out) return OFX_EINVAL;
  const int blocks = (int)mse_blocks(n);
  const float s = (float)(2.0 / (double)n);
  mse_grad_kernel<<<blocks, MSE_THREADS, 0, ofx_stream(stream)>>>(y, target, dy, partials, n, s);
  OFX_LAUNCH_CHECK();
  mse_finish_kernel<<<1, MSE_THREADS, 0, ofx_stream(stream)>>>(partials, blocks, loss_out, n);
  OFX_LAUNCH_CHECK();
  return OFX_OK;
}

// krylov_basis.hpp — the two basis kernels of a Gram-Schmidt step, shared by gmres.hip (restarted GMRES and
// spl_vector_dots_dev), eigsh.hip (thick-restart Lanczos) and lobpcg.hip (LOBPCG): k inner products against a basis in
// ONE pass (dots_kernel / dots_launch) and the update w = ((w - c_0 v_0) - c_1 v_1) - ... in one pass (update_kernel);
// and the two first levels the eigensolvers fold to a scalar, a norm and a pair's residual (norm_kernel,
// residual_kernel).  The arithmetic is the fold of krylov_fold.hpp: every value is what k separate inner products and
// k separate updates would give, bit for bit.  Device code and the host code that launches it; included by those
// three files only (lobpcg.hip also through basis_pair.hpp, the same step in the inner product of a mass matrix).
#pragma once

#include "krylov_fold.hpp"

namespace spl {
namespace {

// Columns of the basis per lane_tree round of dots_kernel.  Tuned: SPL_GMRES_DOTS_BATCH = 2, 4 or 8
// chooses another width for a measurement; the bits do not depend on it.
constexpr int kDotsBatch = 4;

__device__ inline Val<1> scaled(double s, Val<1> a) { return Val<1>{s * a.re}; }
__device__ inline Val<2> scaled(double s, Val<2> a) { return Val<2>{s * a.re, s * a.im}; }
__device__ inline Val<1> over(Val<1> a, double d) { return Val<1>{a.re / d}; }
__device__ inline Val<2> over(Val<2> a, double d) { return Val<2>{a.re / d, a.im / d}; }
__device__ inline double imag_of(Val<1>) { return 0.0; }
__device__ inline double imag_of(Val<2> a) { return a.im; }

// ---- k inner products in one pass ------------------------------------------------------------------------------------
// part[(col * VW + p) * stride + c] = plane p of chunk c of <V[:, col], w>.  A workgroup takes whole chunks; it loads its
// 16 entries per lane of w once and walks the columns B at a time: B * VW lane sums, one lane_tree round for them.  A
// column's sums are dot_kernel's: from +0.0, the entries t, t + 256, ... in ascending order, the same product.
template <int VW, int B>
__global__ __launch_bounds__(kLanes) void dots_kernel(const int *stop, int64_t n, int k, const double *__restrict__ V,
                                                      int64_t ldv, const double *__restrict__ w, double *part,
                                                      int64_t stride) {
  if (stop && *stop) return;
  __shared__ double lds[B * VW * kLanes];
  const int t = threadIdx.x;
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t base = c * kChunk + t;
    const bool full = n - c * kChunk >= kChunk;
    Val<VW> wv[kSteps];
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      const int64_t i = base + (int64_t)s * kLanes;
      wv[s] = (full || i < n) ? load_val<VW>(w, i) : Val<VW>();
    }
    for (int col0 = 0; col0 < k; col0 += B) {
      double acc[B * VW];
#pragma unroll
      for (int v = 0; v < B * VW; ++v) acc[v] = 0.0;
#pragma unroll
      for (int b = 0; b < B; ++b) {
        if (col0 + b < k) {
          const double *col = V + (size_t)(col0 + b) * (size_t)ldv * VW;
#pragma unroll
          for (int s = 0; s < kSteps; ++s) {
            const int64_t i = base + (int64_t)s * kLanes;
            if (full || i < n) accumulate(acc + b * VW, mul(conj_of(load_val<VW>(col, i)), wv[s]));
          }
        }
      }
      lane_tree<B * VW>(acc, lds);
      if (t == 0) {
#pragma unroll
        for (int b = 0; b < B; ++b)
          if (col0 + b < k)
#pragma unroll
            for (int p = 0; p < VW; ++p) part[((int64_t)(col0 + b) * VW + p) * stride + c] = acc[b * VW + p];
      }
    }
  }
}

inline int dots_batch() {
  const char *e = getenv("SPL_GMRES_DOTS_BATCH");
  const long v = e ? atol(e) : 0;
  return v == 2 || v == 4 || v == 8 ? (int)v : kDotsBatch;
}

// the first level, the middle levels and the last one of k inner products: `out` receives k entries.  n > 0
template <int VW>
int dots_launch(const int *stop, int64_t n, int k, const double *V, int64_t ldv, const double *w, double *out,
                double *scratch, hipStream_t s) {
  const int64_t c1 = chunks_of(n);
  const dim3 grid(chunk_grid(n)), block(kLanes);
  switch (dots_batch()) {
    case 2: hipLaunchKernelGGL((dots_kernel<VW, 2>), grid, block, 0, s, stop, n, k, V, ldv, w, scratch, c1); break;
    case 8: hipLaunchKernelGGL((dots_kernel<VW, 8>), grid, block, 0, s, stop, n, k, V, ldv, w, scratch, c1); break;
    default: hipLaunchKernelGGL((dots_kernel<VW, 4>), grid, block, 0, s, stop, n, k, V, ldv, w, scratch, c1); break;
  }
  const Partials P = middle_levels(stop, n, k * VW, scratch, s);
  hipLaunchKernelGGL(fold_kernel, dim3(1, k * VW), block, 0, s, stop, (int64_t)P.count, P.p, P.stride, out, (int64_t)1);
  return P.middle + 2;
}

// ---- the update of a step ---------------------------------------------------------------------------------------------
// w = ((w - c_0 v_0) - c_1 v_1) - ... over ncols columns, a product and a difference per term; NORM: the partials of
// Re<w,w> of the result to part[chunk].  stop: the flag of the caller's status block that ends a cycle
template <int VW, bool NORM>
__global__ __launch_bounds__(kLanes) void update_kernel(const int *stop, int64_t n, int ncols,
                                                        const double *__restrict__ V, int64_t ldv,
                                                        const double *__restrict__ coef, double *__restrict__ w,
                                                        double *part) {
  if (*stop) return;
  __shared__ double lds[kLanes];
  const int t = threadIdx.x;
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t base = c * kChunk + t;
    const bool full = n - c * kChunk >= kChunk;
    Val<VW> wv[kSteps];
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      const int64_t i = base + (int64_t)s * kLanes;
      wv[s] = (full || i < n) ? load_val<VW>(w, i) : Val<VW>();
    }
    for (int col = 0; col < ncols; ++col) {
      const Val<VW> cf = load_val<VW>(coef, col);
      const double *v = V + (size_t)col * (size_t)ldv * VW;
#pragma unroll
      for (int s = 0; s < kSteps; ++s) {
        const int64_t i = base + (int64_t)s * kLanes;
        if (full || i < n) wv[s] = sub(wv[s], mul(cf, load_val<VW>(v, i)));
      }
    }
    double acc[1] = {0.0};
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      const int64_t i = base + (int64_t)s * kLanes;
      if (full || i < n) {
        store_val(w, i, wv[s]);
        if (NORM) acc[0] = acc[0] + mul(conj_of(wv[s]), wv[s]).re;
      }
    }
    if (NORM) {
      lane_tree<1>(acc, lds);
      if (t == 0) part[c] = acc[0];
    }
  }
}

// ---- the first levels of the eigensolvers' scalars ---------------------------------------------------------------------
// partials of Re<v,v>
template <int VW>
__global__ __launch_bounds__(kLanes) void norm_kernel(int64_t n, const double *__restrict__ v, double *part) {
  chunk_partials<1>(n, part, 0, [&](int64_t i, double *acc) {
    const Val<VW> vi = load_val<VW>(v, i);
    acc[0] = acc[0] + mul(conj_of(vi), vi).re;
  });
}

// r = ax - lambda x, one product part by part and one difference per entry, stored when r is given; partials of Re<r,r>
template <int VW>
__global__ __launch_bounds__(kLanes) void residual_kernel(int64_t n, const double *__restrict__ ax,
                                                          const double *__restrict__ x, double lambda,
                                                          double *__restrict__ r, double *part) {
  chunk_partials<1>(n, part, 0, [&](int64_t i, double *acc) {
    const Val<VW> ri = sub(load_val<VW>(ax, i), scaled(lambda, load_val<VW>(x, i)));
    if (r) store_val(r, i, ri);
    acc[0] = acc[0] + mul(conj_of(ri), ri).re;
  });
}

// ---- the launches of a step --------------------------------------------------------------------------------------------
// Classical Gram-Schmidt done twice of w against the first k columns of V (leading dimension n): the coefficients of
// the passes to c1 and c2 (k entries each), the partials of <w,w> of the result folded until the last level is left.
// *launches grows by the kernels.  n > 0
template <int VW>
Partials orthogonalise_twice(const int *stop, int64_t n, int k, const double *V, double *w, double *c1, double *c2,
                             double *scratch, unsigned chunked, hipStream_t s, int64_t *launches) {
  *launches += dots_launch<VW>(stop, n, k, V, n, w, c1, scratch, s);
  hipLaunchKernelGGL((update_kernel<VW, false>), dim3(chunked), dim3(kLanes), 0, s, stop, n, k, V, n, (const double *)c1, w,
                     scratch);
  *launches += dots_launch<VW>(stop, n, k, V, n, w, c2, scratch, s);
  hipLaunchKernelGGL((update_kernel<VW, true>), dim3(chunked), dim3(kLanes), 0, s, stop, n, k, V, n, (const double *)c2, w,
                     scratch);
  const Partials P = middle_levels(stop, n, 1, scratch, s);
  *launches += P.middle + 2;
  return P;
}

}  // namespace
}  // namespace spl

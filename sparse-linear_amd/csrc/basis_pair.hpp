// basis_pair.hpp — the kernels of a Gram-Schmidt step in the inner product <u,v>_B = <u, B v>, where every column of the
// basis is kept together with its image under B (lobpcg.hip with a mass matrix, and spl_vector_update_pair_dev): the
// update of a column AND of its image by the same coefficients, with the partials of Re<w, bw> of the results, in ONE
// pass (update_pair_kernel); the partials of Re<a,b> alone (pair_norm_kernel); and the residual of a pencil,
// r = ax - theta bx (pencil_residual_kernel).  The arithmetic is that of krylov_basis.hpp term by term and the fold of
// krylov_fold.hpp: Re<w, bw> is the real part of spl_vector_dot_dev(w, bw) bit for bit.  Device code and the host code
// that launches it; included by lobpcg.hip only.
#pragma once

#include "krylov_basis.hpp"

namespace spl {
namespace {

// w = ((w - c_0 v_0) - c_1 v_1) - ... and bw = ((bw - c_0 (Bv)_0) - c_1 (Bv)_1) - ... over ncols columns, ascending, the
// same coefficients for both, a product and a difference per term (update_kernel's).  A lane keeps its 16 entries of w
// and of bw in registers (64 doubles when complex) and the columns of V and BV stream past them.  NORM: the partials of
// Re<w, bw> of the results to part[chunk]: lane t adds its 16 products in ascending order from +0.0, then the tree
// (dot_kernel's real plane).  stop: the flag of the caller's status block that ends a cycle, or nullptr
template <int VW, bool NORM>
__global__ __launch_bounds__(kLanes) void update_pair_kernel(const int *stop, int64_t n, int ncols,
                                                             const double *__restrict__ V, int64_t ldv,
                                                             const double *__restrict__ BV, int64_t ldbv,
                                                             const double *__restrict__ coef, double *__restrict__ w,
                                                             double *__restrict__ bw, double *part) {
  if (stop && *stop) return;
  __shared__ double lds[kLanes];
  const int t = threadIdx.x;
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t base = c * kChunk + t;
    const bool full = n - c * kChunk >= kChunk;
    Val<VW> wv[kSteps], bv[kSteps];
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      const int64_t i = base + (int64_t)s * kLanes;
      const bool in = full || i < n;
      wv[s] = in ? load_val<VW>(w, i) : Val<VW>();
      bv[s] = in ? load_val<VW>(bw, i) : Val<VW>();
    }
    for (int col = 0; col < ncols; ++col) {
      const Val<VW> cf = load_val<VW>(coef, col);
      const double *v = V + (size_t)col * (size_t)ldv * VW;
      const double *b = BV + (size_t)col * (size_t)ldbv * VW;
#pragma unroll
      for (int s = 0; s < kSteps; ++s) {
        const int64_t i = base + (int64_t)s * kLanes;
        if (full || i < n) {
          wv[s] = sub(wv[s], mul(cf, load_val<VW>(v, i)));
          bv[s] = sub(bv[s], mul(cf, load_val<VW>(b, i)));
        }
      }
    }
    double acc[1] = {0.0};
#pragma unroll
    for (int s = 0; s < kSteps; ++s) {
      const int64_t i = base + (int64_t)s * kLanes;
      if (full || i < n) {
        store_val(w, i, wv[s]);
        store_val(bw, i, bv[s]);
        if (NORM) acc[0] = acc[0] + mul(conj_of(wv[s]), bv[s]).re;
      }
    }
    if (NORM) {
      lane_tree<1>(acc, lds);
      if (t == 0) part[c] = acc[0];
    }
  }
}

// partials of Re<a,b>: the real plane of dot_kernel
template <int VW>
__global__ __launch_bounds__(kLanes) void pair_norm_kernel(int64_t n, const double *__restrict__ a,
                                                           const double *__restrict__ b, double *part) {
  chunk_partials<1>(n, part, 0, [&](int64_t i, double *acc) {
    acc[0] = acc[0] + mul(conj_of(load_val<VW>(a, i)), load_val<VW>(b, i)).re;
  });
}

// r = ax - theta bx, one product part by part and one difference per entry, stored when r is given; partials of
// Re<r,r>: residual_kernel with bx where x is
template <int VW>
__global__ __launch_bounds__(kLanes) void pencil_residual_kernel(int64_t n, const double *__restrict__ ax,
                                                                 const double *__restrict__ bx, double theta,
                                                                 double *__restrict__ r, double *part) {
  chunk_partials<1>(n, part, 0, [&](int64_t i, double *acc) {
    const Val<VW> ri = sub(load_val<VW>(ax, i), scaled(theta, load_val<VW>(bx, i)));
    if (r) store_val(r, i, ri);
    acc[0] = acc[0] + mul(conj_of(ri), ri).re;
  });
}

// the paired update of w and bw against k columns (coef: k entries) and, with `norm`, the partials of Re<w, bw> of the
// results in scratch (first level).  n > 0
template <int VW>
void update_pair_launch(const int *stop, int64_t n, int k, const double *V, int64_t ldv, const double *BV, int64_t ldbv,
                        const double *coef, double *w, double *bw, bool norm, double *scratch, unsigned chunked,
                        hipStream_t s) {
  if (norm)
    hipLaunchKernelGGL((update_pair_kernel<VW, true>), dim3(chunked), dim3(kLanes), 0, s, stop, n, k, V, ldv, BV, ldbv, coef,
                       w, bw, scratch);
  else
    hipLaunchKernelGGL((update_pair_kernel<VW, false>), dim3(chunked), dim3(kLanes), 0, s, stop, n, k, V, ldv, BV, ldbv,
                       coef, w, bw, scratch);
}

}  // namespace
}  // namespace spl

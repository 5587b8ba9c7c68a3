// precond.hpp — the preconditioner CG, BiCGSTAB (krylov.hip) and GMRES (gmres.hip) apply: borrowed triangular solves
// around a diagonal, or an AMG cycle.  Device code and the host code that launches it; included by those two files only.
#pragma once

#include "krylov_fold.hpp"

namespace spl {
namespace {

// out = d (.) in, entry by entry; in may be out.  stop: the flag of the caller's status block that ends its work
template <int VW>
__global__ __launch_bounds__(kLanes) void diag_kernel(const int *stop, int64_t n, const double *d, const double *in,
                                                      double *out) {
  if (*stop) return;
  int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kLanes;
  for (; i < n; i += stride) store_val(out, i, mul(load_val<VW>(d, i), load_val<VW>(in, i)));
}

// The parts are borrowed, of the solver's size, value kind and device (abi.hip checked); nullptr: the identity
struct Preconditioner {
  TriSolver *T1 = nullptr, *T2 = nullptr;
  const double *d_mid = nullptr;
  Amg *amg = nullptr;  // set: the three parts above are not

  bool set() const { return T1 || T2 || d_mid || amg; }
  int64_t flags() const { return (T1 ? 2 : 0) | (d_mid ? 4 : 0) | (T2 ? 8 : 0) | (amg ? 16 : 0); }  // of info[2]
  void set_parts(TriSolver *t1, const double *mid, TriSolver *t2) {
    T1 = t1;
    d_mid = mid;
    T2 = t2;
    amg = nullptr;
  }
  void set_amg(Amg *M) {
    T1 = T2 = nullptr;
    d_mid = nullptr;
    amg = M;
  }

  // out = T2^-1 (d_mid (.) (T1^-1 in)), or the AMG cycle of `in`, enqueued on s; called only when a part is set.
  // *launches grows by the kernels.  The solves and the cycle do not read the status block: they write `out` and
  // their own vectors only, which nothing reads once the flag `stop` of the kernels around them is set
  template <int VW>
  int apply(const int *stop, int64_t n, const double *in, double *out, unsigned flat_grid, hipStream_t s,
            int64_t *launches) const {
    if (amg) {
      int64_t enqueued = 0;
      const int e = amg_apply(amg, in, out, s, &enqueued);
      *launches += enqueued;
      return e;
    }
    const double *cur = in;
    int64_t info[8];
    if (T1) {
      const int e = trisolve_solve(T1, SPL_OP_n, 1, cur, n, out, n, s);
      if (e != SPL_OK) return e;
      trisolve_info(T1, info);
      *launches += info[3];
      cur = out;
    }
    if (d_mid) {
      hipLaunchKernelGGL((diag_kernel<VW>), dim3(flat_grid), dim3(kLanes), 0, s, stop, n, d_mid, cur, out);
      ++*launches;
      cur = out;
    }
    if (T2) {
      const int e = trisolve_solve(T2, SPL_OP_n, 1, cur, n, out, n, s);
      if (e != SPL_OK) return e;
      trisolve_info(T2, info);
      *launches += info[3];
    }
    return SPL_OK;
  }
};

}  // namespace
}  // namespace spl

// lobpcg.hip — LOBPCG on device handles: a block eigensolver with the preconditioner inside the iteration, Double and
// packed Complex Double (real symmetric and complex Hermitian).
//
// The method is written out in include/sparse_linear_hip.h ("LOBPCG on handles"); this file issues it.  The basis
// S = [X | P | W] (3 block columns) is kept ORTHONORMAL by classical Gram-Schmidt done twice on the one-pass kernels of
// krylov_basis.hpp, so the Ritz problem is a standard Hermitian one: T = S^H (A S) by spl_vector_gram_dev's kernel
// (gram.hip), diagonalised and ordered on the host by the Ritz step of ritz_jacobi.hpp, and
// [X' | P'] = S [C | C without its X rows] by the in-place rotation of eigsh.hip, real or complex.  Rank deficiency is
// decided on the device without a synchronisation per column: a column whose norm after the two passes is 0, not
// finite, or at most 2^-40 of its norm before is written as zeros and flagged; a zero column contributes +0.0 terms
// only, so the launch sequence of an iteration is the same whatever drops, and the host removes the flagged rows and
// columns from T.  Two synchronisations per iteration: the residual norms; T and the flags.  No captured graph, no
// floating-point atomic, no kernel waits for another workgroup.
//
// With a mass matrix (spl_lobpcg_set_mass) the same method runs in the inner product <u,v>_B = <u, B v> for
// A x = lambda B x: B S is kept beside S and A S, a column is settled together with its image under B by the paired
// update of basis_pair.hpp, the residual is that of the pencil and the rotation is applied to B S too.  Every such step
// is behind `if (B)`: without a mass matrix the kernels, their order and the tables are what they were.
#include <algorithm>
#include <cmath>
#include <vector>

#include "basis_pair.hpp"
#include "krylov_basis.hpp"
#include "ritz_jacobi.hpp"
#include "solver_core.hpp"

namespace spl {

namespace {

constexpr double kDropRatio = 0x1p-40;  // eta2 <= kDropRatio * eta0: the column was in the span of those before it

struct LStatus {
  int zero;  // never set: the flag the shared kernels of a step read
  int spare[3];
};

// in doubles from the start of the block; b = block, m = 3 b.  G and Z first: packed pairs are stored whole
struct LTables {
  double *G;         // m x m entries: S^H (A S), column major
  double *Z;         // m x 2 b entries: the rotation
  double *c1, *c2;   // the coefficients of the two passes: m entries each
  double *eta0;      // m: Re<w,w> of a column before its passes
  double *scale;     // m: its norm after them
  double *res;       // b: Re<r,r>
};
inline size_t ltable_doubles(int b) { return (size_t)30 * b * b + (size_t)19 * b; }
inline LTables ltables_at(double *base, int b) {
  LTables T;
  T.G = base;
  T.Z = T.G + (size_t)18 * b * b;
  T.c1 = T.Z + (size_t)12 * b * b;
  T.c2 = T.c1 + 6 * b;
  T.eta0 = T.c2 + 6 * b;
  T.scale = T.eta0 + 3 * b;
  T.res = T.scale + 3 * b;
  return T;
}

// ONE workgroup behind the passes of a column: eta2 from the last partials of Re<w,w>, eta0 from the table, the flag
// (0 kept, 1 dropped, 2 not finite) and what a kept column is divided by
__global__ __launch_bounds__(kLanes) void decide_kernel(const double *part, int count, const double *eta0sq,
                                                        double *scale, int *flag) {
  const double sum = sum_partials(part, count);
  if (threadIdx.x != 0) return;
  const double e2 = sqrt(sum), e0 = sqrt(*eta0sq);
  *scale = e2;
  if (!isfinite(e0) || !isfinite(e2)) *flag = 2;
  else if (e2 == 0.0 || e2 <= kDropRatio * e0) *flag = 1;
  else *flag = 0;
}

// The same behind the passes of a column in the inner product of a mass matrix: q2 = Re<s, B s> from the last partials,
// q0 from the table.  A negative q says that B is not positive definite on the column: dropped
__global__ __launch_bounds__(kLanes) void decide_pair_kernel(const double *part, int count, const double *q0p,
                                                             double *scale, int *flag) {
  const double q2 = sum_partials(part, count);
  if (threadIdx.x != 0) return;
  const double q0 = *q0p;
  const double e2 = sqrt(q2), e0 = sqrt(q0);
  *scale = e2;
  if (!isfinite(q0) || !isfinite(q2)) *flag = 2;
  else if (q0 < 0.0 || q2 < 0.0) *flag = 1;
  else if (e2 == 0.0 || e2 <= kDropRatio * e0) *flag = 1;
  else *flag = 0;
}

// w = w / scale part by part, or zeros when the column is flagged
template <int VW>
__global__ __launch_bounds__(kLanes) void settle_kernel(int64_t n, const int *flag, const double *scale, double *w) {
  const bool drop = *flag != 0;
  const double by = *scale;
  int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kLanes;
  for (; i < n; i += stride) store_val(w, i, drop ? Val<VW>() : over(load_val<VW>(w, i), by));
}

}  // namespace

// ---- the solver object (the shared part: solver_core.hpp) ---------------------------------------------------------------
// with a mass matrix 3 block + 1 more (`mass`): 10 block + 2 in all
struct Lobpcg : SolverCore {  // work: 7 block + 1 vectors: S (3 block), A S (3 block), R (block), one product
  int block;
  Preconditioner pre;
  const Matrix *B = nullptr;     // the mass matrix of A x = lambda B x, borrowed; nullptr: the standard problem
  DBuf<double> mass;             // with B: 3 block + 1 vectors, B S and a second product
  int64_t last_mass_columns = 0;  // columns multiplied by B in the last solve
  DBuf<double> tables;
  DBuf<int> flags;               // 3 block
  StatusBlock<LStatus> status;   // behind the pinned copy: G, Z, res and the flags of the host
  Lobpcg(const Matrix *A, int b)
      : SolverCore(kLobpcgMagic, A, (size_t)7 * b + 1, fold_scratch(A->nrows_local, 3 * b * A->vw)), block(b),
        tables(ltable_doubles(b)), flags((size_t)3 * b),
        status(((size_t)30 * b * b + (size_t)b) * sizeof(double) + (size_t)3 * b * sizeof(int)) {
    bytes += ltable_doubles(b) * sizeof(double) + (size_t)3 * b * sizeof(int) + sizeof(LStatus);
  }
  double *host_g() const { return reinterpret_cast<double *>(status.pinned + 1); }
  double *host_z() const { return host_g() + (size_t)18 * block * block; }
  double *host_res() const { return host_z() + (size_t)12 * block * block; }
  int *host_flags() const { return reinterpret_cast<int *>(host_res() + block); }
  size_t mass_doubles() const { return ((size_t)3 * block + 1) * (size_t)n * (size_t)vw; }
};

// A: whole, square and Hermitian, 1 <= block <= 42 (the caller checked)
int lobpcg_create(const Matrix *A, int block, Lobpcg **out) {
  *out = new Lobpcg(A, block);
  return SPL_OK;
}

void lobpcg_set_preconditioner(Lobpcg *L, TriSolver *T1, const double *d_mid, TriSolver *T2) {
  std::lock_guard<std::mutex> hold(L->lock);
  L->pre.set_parts(T1, d_mid, T2);
}

void lobpcg_set_preconditioner_amg(Lobpcg *L, Amg *M) {
  std::lock_guard<std::mutex> hold(L->lock);
  L->pre.set_amg(M);
}

// B: whole, square, Hermitian and of L's size, value kind and device (the caller checked), or nullptr
void lobpcg_set_mass(Lobpcg *L, const Matrix *B) {
  std::lock_guard<std::mutex> hold(L->lock);
  if (B && !L->B) {
    L->mass.alloc(L->mass_doubles());
    L->bytes += L->mass_doubles() * sizeof(double);
  } else if (!B && L->B) {
    L->mass.release();
    L->bytes -= L->mass_doubles() * sizeof(double);
  }
  L->B = B;
  L->last_mass_columns = 0;
}

int lobpcg_block(const Lobpcg *L) { return L->block; }

namespace {

// One solve's launches; everything is enqueued on s
template <int VW>
struct LRun : RunCore {
  Lobpcg *L;
  int b;
  LTables T;
  int *flags;
  const int *never;  // the flag that is never set
  const Matrix *B;   // the mass matrix, or nullptr
  int64_t spmv_columns = 0, mass_columns = 0, applications = 0, sweeps_most = 0, dropped = 0, syncs = 0;
  std::vector<double> theta;  // of the block's columns

  LRun(Lobpcg *l, hipStream_t stream)
      : RunCore(*l, stream), L(l), b(l->block), T(ltables_at(l->tables.get(), l->block)), flags(l->flags.get()),
        never(&l->status.device.get()->zero), B(l->B), theta((size_t)l->block, 0.0) {}

  double *basis(int j) const { return L->vec(j); }               // S
  double *image(int j) const { return L->vec(3 * b + j); }       // A S
  double *residual(int j) const { return L->vec(6 * b + j); }    // R, when a preconditioner reads it
  double *product() const { return L->vec(7 * b); }
  double *mass_image(int j) const { return L->mass.get() + (size_t)j * (size_t)n * VW; }  // B S
  double *mass_product() const { return mass_image(3 * b); }

  void sync() {
    SPL_HIP(hipStreamSynchronize(s));
    ++syncs;
  }

  // Re<v,v> of n entries folded to *out
  void norm_to(const double *v, double *out) {
    hipLaunchKernelGGL((norm_kernel<VW>), dim3(chunked), dim3(kLanes), 0, s, n, v, scratch);
    ++launches;
    fold_to(out);
  }

  // column c of S against the c columns before it: the norm before, the two passes, the decision, the division
  void settle_column(int c) {
    if (B) return settle_column_mass(c);
    double *w = basis(c);
    norm_to(w, T.eta0 + c);
    Partials P;
    if (c > 0) {
      P = orthogonalise_twice<VW>(never, n, c, basis(0), w, T.c1, T.c2, scratch, chunked, s, &launches);
    } else {
      hipLaunchKernelGGL((norm_kernel<VW>), dim3(chunked), dim3(kLanes), 0, s, n, (const double *)w, scratch);
      ++launches;
      P = last_level();
    }
    hipLaunchKernelGGL(decide_kernel, dim3(1), dim3(kLanes), 0, s, P.p, P.count, (const double *)(T.eta0 + c), T.scale + c,
                       flags + c);
    hipLaunchKernelGGL((settle_kernel<VW>), dim3(flat), dim3(kLanes), 0, s, n, (const int *)(flags + c),
                       (const double *)(T.scale + c), w);
    launches += 2;
  }

  // Re<a,b> of n entries: its first level in scratch
  void pair_norm(const double *a, const double *bv) {
    hipLaunchKernelGGL((pair_norm_kernel<VW>), dim3(chunked), dim3(kLanes), 0, s, n, a, bv, scratch);
    ++launches;
  }

  // settle_column in the inner product of B: s_c and (B s)_c against the columns before them, the coefficients from
  // B S, both updated in one pass that also leaves Re<s_c, (B s)_c>
  void settle_column_mass(int c) {
    double *w = basis(c), *bw = mass_image(c);
    pair_norm(w, bw);
    fold_to(T.eta0 + c);
    Partials P;
    if (c > 0) {
      launches += dots_launch<VW>(never, n, c, mass_image(0), n, w, T.c1, scratch, s);
      update_pair_launch<VW>(never, n, c, basis(0), n, mass_image(0), n, T.c1, w, bw, false, scratch, chunked, s);
      launches += dots_launch<VW>(never, n, c, mass_image(0), n, w, T.c2, scratch, s);
      update_pair_launch<VW>(never, n, c, basis(0), n, mass_image(0), n, T.c2, w, bw, true, scratch, chunked, s);
      launches += 2;
    } else {
      pair_norm(w, bw);
    }
    P = last_level();
    hipLaunchKernelGGL(decide_pair_kernel, dim3(1), dim3(kLanes), 0, s, P.p, P.count, (const double *)(T.eta0 + c),
                       T.scale + c, flags + c);
    hipLaunchKernelGGL((settle_kernel<VW>), dim3(flat), dim3(kLanes), 0, s, n, (const int *)(flags + c),
                       (const double *)(T.scale + c), w);
    hipLaunchKernelGGL((settle_kernel<VW>), dim3(flat), dim3(kLanes), 0, s, n, (const int *)(flags + c),
                       (const double *)(T.scale + c), bw);
    launches += 3;
  }

  // X' behind a rotation is orthonormal to the rounding of the rotation only, and that loss adds up over the iterations
  // (1.2e-13 after 56 of them on the 12 x 12 grid, which biases theta by as much, relatively).  So X is settled again,
  // and A X receives the same coefficients, the same division and the same zeros: it stays the product of X
  void settle_block() {
    for (int j = 0; j < b; ++j) {
      settle_column(j);
      if (j > 0) {
        hipLaunchKernelGGL((update_kernel<VW, false>), dim3(chunked), dim3(kLanes), 0, s, never, n, j,
                           (const double *)image(0), n, (const double *)T.c1, image(j), scratch);
        hipLaunchKernelGGL((update_kernel<VW, false>), dim3(chunked), dim3(kLanes), 0, s, never, n, j,
                           (const double *)image(0), n, (const double *)T.c2, image(j), scratch);
        launches += 2;
      }
      hipLaunchKernelGGL((settle_kernel<VW>), dim3(flat), dim3(kLanes), 0, s, n, (const int *)(flags + j),
                         (const double *)(T.scale + j), image(j));
      ++launches;
    }
  }

  // r_i = ax - theta_i x_i (with a mass matrix: ax - theta_i bx) to `out` (nullptr: not stored) and Re<r_i,r_i> to
  // res[i]; ax: A x_i, bx: B x_i
  void residual_of(int i, const double *ax, const double *bx, double *out) {
    if (B)
      hipLaunchKernelGGL((pencil_residual_kernel<VW>), dim3(chunked), dim3(kLanes), 0, s, n, ax, bx, theta[i], out, scratch);
    else
      hipLaunchKernelGGL((residual_kernel<VW>), dim3(chunked), dim3(kLanes), 0, s, n, ax, (const double *)basis(i), theta[i],
                         out, scratch);
    ++launches;
    fold_to(T.res + i);
  }

  // The close on the first mc columns of S: T = S^H (A S), the flags, Jacobi, the order, and the rotation that leaves
  // kout columns (b: X' alone; 2 b: [X' | P']).  count_from: the first column whose drop is counted.  *reason >= 0
  // ends the solve; -1: go on.  Synchronises once
  int close(int mc, int kout, int which, int count_from, int *reason) {
    *reason = -1;
    int e = vector_gram(L->device, n, VW, mc, mc, basis(0), n, image(0), n, T.G, mc, 1, s, &launches);
    if (e != SPL_OK) return e;
    double *G = L->host_g();
    int *flag = L->host_flags();
    SPL_HIP(hipMemcpyAsync(G, T.G, (size_t)mc * mc * VW * sizeof(double), hipMemcpyDeviceToHost, s));
    SPL_HIP(hipMemcpyAsync(flag, flags, (size_t)3 * b * sizeof(int), hipMemcpyDeviceToHost, s));
    sync();
    std::vector<int> kept;
    for (int j = 0; j < mc; ++j) {
      if (flag[j] == 2 || (j < b && flag[j] != 0)) return not_finite(reason);  // a column of X never drops
      if (flag[j] == 0) kept.push_back(j);
      else if (j >= count_from) ++dropped;
    }
    const int mp = (int)kept.size();
    std::vector<double> Tm((size_t)mp * mp * VW), Y((size_t)mp * mp * VW);
    for (int a = 0; a < mp; ++a)
      for (int c = a; c < mp; ++c) {
        const double *g = G + ((size_t)kept[c] * mc + kept[a]) * VW;  // the upper triangle: i <= j
        if (!std::isfinite(g[0]) || (VW == 2 && a != c && !std::isfinite(g[1]))) return not_finite(reason);
        if (VW == 1) {
          Tm[(size_t)a * mp + c] = Tm[(size_t)c * mp + a] = g[0];
        } else {
          Tm[2 * ((size_t)a * mp + c)] = Tm[2 * ((size_t)c * mp + a)] = g[0];
          const double gi = a == c ? 0.0 : g[1];
          Tm[2 * ((size_t)a * mp + c) + 1] = gi;
          Tm[2 * ((size_t)c * mp + a) + 1] = a == c ? 0.0 : -gi;
        }
      }
    std::vector<int> order(mp);
    const int sweeps = ritz_step(mp, VW, which, Tm.data(), Y.data(), order.data());
    if (sweeps < 0) return not_finite(reason);
    if (sweeps > sweeps_most) sweeps_most = sweeps;
    auto value = [&](int i) { return Tm[((size_t)i * mp + i) * VW]; };
    // Z: mc x kout, column major; rows of flagged columns and, in the second block, the rows of X are +0.0
    double *Z = L->host_z();
    for (size_t q = 0; q < (size_t)mc * kout * VW; ++q) Z[q] = 0.0;
    for (int i = 0; i < kout; ++i) {
      const int col = order[i < b ? i : i - b];
      for (int a = 0; a < mp; ++a) {
        if (i >= b && kept[a] < b) continue;
        for (int p = 0; p < VW; ++p) Z[((size_t)i * mc + kept[a]) * VW + p] = Y[((size_t)a * mp + col) * VW + p];
      }
    }
    SPL_HIP(hipMemcpyAsync(T.Z, Z, (size_t)mc * kout * VW * sizeof(double), hipMemcpyHostToDevice, s));
    if ((e = vector_rotate(n, VW, mc, kout, basis(0), n, T.Z, mc, nullptr, 0, s, VW == 2)) != SPL_OK) return e;
    if ((e = vector_rotate(n, VW, mc, kout, image(0), n, T.Z, mc, nullptr, 0, s, VW == 2)) != SPL_OK) return e;
    launches += 2;
    if (B) {
      if ((e = vector_rotate(n, VW, mc, kout, mass_image(0), n, T.Z, mc, nullptr, 0, s, VW == 2)) != SPL_OK) return e;
      ++launches;
    }
    for (int i = 0; i < b; ++i) theta[i] = value(order[i]);
    settle_block();
    return SPL_OK;
  }
  static int not_finite(int *reason) {
    *reason = 3;
    return SPL_OK;
  }

  int solve(int nev, int which, double tol, double atol, int64_t max_iter, const double *d_X0, int64_t ldx0,
            double *values, double *d_vectors, int64_t ldx, double *residuals, int64_t result[8], double *history) {
    int e;
    int64_t iterations = 0;
    const size_t column = (size_t)n * VW * sizeof(double);
    auto done = [&](int reason, int pairs) {
      result[0] = reason;
      result[1] = iterations;
      result[2] = spmv_columns;
      result[3] = pairs;
      result[4] = applications;
      result[5] = sweeps_most;
      result[6] = dropped;
      result[7] = syncs;
      return SPL_OK;
    };
    // X and the pairs' true residuals; synchronises
    auto finish = [&](int reason) {
      for (int i = 0; i < nev; ++i) {
        SPL_HIP(hipMemcpyAsync(d_vectors + (size_t)i * (size_t)ldx * VW, basis(i), column, hipMemcpyDeviceToDevice, s));
        values[i] = theta[i];
        const int st = launch_spmv(L->A, basis(i), product(), 0, s);
        if (st != SPL_OK) return st;
        ++spmv_columns;
        ++launches;
        if (B) {
          const int sb = launch_spmv(B, basis(i), mass_product(), 0, s);
          if (sb != SPL_OK) return sb;
          ++mass_columns;
          ++launches;
        }
        residual_of(i, product(), B ? mass_product() : nullptr, nullptr);
      }
      const int st = launch_status("lobpcg finish");
      if (st != SPL_OK) return st;
      SPL_HIP(hipMemcpyAsync(L->host_res(), T.res, (size_t)nev * sizeof(double), hipMemcpyDeviceToHost, s));
      sync();
      for (int i = 0; i < nev; ++i) residuals[i] = sqrt(L->host_res()[i]);
      return done(reason, nev);
    };

    // ---- start: X = orthonormalised X0, P = 0, Rayleigh-Ritz on X alone
    SPL_HIP(hipMemsetAsync(L->status.device.get(), 0, sizeof(LStatus), s));
    SPL_HIP(hipMemsetAsync(flags, 0, (size_t)3 * b * sizeof(int), s));
    for (int j = 0; j < b; ++j)
      SPL_HIP(hipMemcpyAsync(basis(j), d_X0 + (size_t)j * (size_t)ldx0 * VW, column, hipMemcpyDeviceToDevice, s));
    SPL_HIP(hipMemsetAsync(basis(b), 0, column * (size_t)b, s));
    if (B) {  // B X by one product; the image of P = 0 is zero
      SPL_HIP(hipMemsetAsync(mass_image(b), 0, column * (size_t)b, s));
      if ((e = launch_spmv_many(B, b, basis(0), n, mass_image(0), n, 0, s)) != SPL_OK) return e;
      mass_columns += b;
      ++launches;
    }
    for (int j = 0; j < b; ++j) settle_column(j);
    if ((e = launch_status("lobpcg start")) != SPL_OK) return e;
    SPL_HIP(hipMemcpyAsync(L->host_flags(), flags, (size_t)3 * b * sizeof(int), hipMemcpyDeviceToHost, s));
    sync();
    bool deficient = false;
    for (int j = 0; j < b; ++j) {
      if (L->host_flags()[j] == 2) return done(3, 0);
      deficient = deficient || L->host_flags()[j] == 1;
    }
    if (deficient) return done(2, 0);
    if ((e = launch_spmv_many(L->A, b, basis(0), n, image(0), n, 0, s)) != SPL_OK) return e;
    spmv_columns += b;
    ++launches;
    int code = -1;
    if ((e = close(b, b, which, b, &code)) != SPL_OK) return e;
    if (code >= 0) return done(code, 0);

    for (int64_t it = 0;; ++it) {
      iterations = it;
      const bool pre = L->pre.set();
      for (int i = 0; i < b; ++i)
        residual_of(i, image(i), B ? mass_image(i) : nullptr, pre ? residual(i) : basis(2 * b + i));
      if ((e = launch_status("lobpcg residuals")) != SPL_OK) return e;
      SPL_HIP(hipMemcpyAsync(L->host_res(), T.res, (size_t)b * sizeof(double), hipMemcpyDeviceToHost, s));
      sync();
      double worst = 0.0;
      bool converged = true, finite = true;
      for (int i = 0; i < b; ++i) {
        const double rn = sqrt(L->host_res()[i]);
        finite = finite && std::isfinite(rn);
        if (i >= nev) continue;
        if (rn > worst) worst = rn;
        const double bound = tol * fabs(theta[i]);
        converged = converged && rn <= (bound > atol ? bound : atol);
      }
      if (!finite) return done(3, 0);
      if (history) history[it] = worst;
      if (converged) return finish(0);
      if (it >= max_iter) return finish(1);
      if (pre) {
        for (int i = 0; i < b; ++i) {
          if ((e = L->pre.template apply<VW>(never, n, residual(i), basis(2 * b + i), flat, s, &launches)) != SPL_OK) return e;
          ++applications;
        }
      }
      if (B) {  // B W by one product; P's image is the rotation's
        if ((e = launch_spmv_many(B, b, basis(2 * b), n, mass_image(2 * b), n, 0, s)) != SPL_OK) return e;
        mass_columns += b;
        ++launches;
      }
      for (int j = b; j < 3 * b; ++j) settle_column(j);  // P, then W
      if ((e = launch_spmv_many(L->A, 2 * b, basis(b), n, image(b), n, 0, s)) != SPL_OK) return e;
      spmv_columns += 2 * b;
      ++launches;
      if ((e = launch_status("lobpcg iteration")) != SPL_OK) return e;
      // iteration 0 has no P: its zero columns are not drops
      if ((e = close(3 * b, 2 * b, which, it == 0 ? 2 * b : b, &code)) != SPL_OK) return e;
      iterations = it + 1;
      if (code >= 0) return done(code, 0);
    }
  }
};

}  // namespace

// arguments checked by the caller; n > 0.  Enqueues on s and synchronises it: the outcome is read back.
int lobpcg_solve(Lobpcg *L, int nev, int which, double tol, double atol, int64_t max_iter, const double *d_X0,
                 int64_t ldx0, double *values, double *d_vectors, int64_t ldx, double *residuals, int64_t result[8],
                 double *history, hipStream_t s) {
  std::lock_guard<std::mutex> hold(L->lock);
  return L->solve_and_record(s, result + 1, [&](auto width, int64_t *launches) {
    LRun<decltype(width)::value> run(L, s);
    const int e = run.solve(nev, which, tol, atol, max_iter, d_X0, ldx0, values, d_vectors, ldx, residuals, result, history);
    *launches = run.launches;
    if (e == SPL_OK) L->last_mass_columns = run.mass_columns;
    return e;
  });
}

void lobpcg_info(Lobpcg *L, int64_t info[8]) {
  std::lock_guard<std::mutex> hold(L->lock);
  L->fill_info(info, L->block, L->pre.flags() | (L->B ? 32 : 0));
  info[7] = L->last_mass_columns;
}

void lobpcg_delete(Lobpcg *L) { delete_object(L); }

// ---- spl_vector_update_pair_dev ---------------------------------------------------------------------------------------------
// w and bw against the k columns of V and BV by the coefficients d_coef, and Re<w, bw> of the results to d_q when it is
// given; enqueues on s.  Arguments checked by the caller.
int vector_update_pair(int device, int64_t n, int vw, int k, const double *d_V, int64_t ldv, const double *d_BV,
                       int64_t ldbv, const double *d_coef, double *d_w, double *d_bw, double *d_q, hipStream_t s) {
  if (n == 0) {
    if (d_q) SPL_HIP(hipMemsetAsync(d_q, 0, sizeof(double), s));  // +0.0
    return SPL_OK;
  }
  DotBlock *block = d_q ? dot_block_take(device, fold_scratch(n, 1)) : nullptr;
  double *scratch = block ? block->buf.get() : nullptr;
  const unsigned chunked = chunk_grid(n);
  if (vw == 1) update_pair_launch<1>(nullptr, n, k, d_V, ldv, d_BV, ldbv, d_coef, d_w, d_bw, d_q != nullptr, scratch, chunked, s);
  else update_pair_launch<2>(nullptr, n, k, d_V, ldv, d_BV, ldbv, d_coef, d_w, d_bw, d_q != nullptr, scratch, chunked, s);
  if (d_q) {
    const Partials P = middle_levels(nullptr, n, 1, scratch, s);
    hipLaunchKernelGGL(fold_kernel, dim3(1, 1), dim3(kLanes), 0, s, (const int *)nullptr, (int64_t)P.count, P.p, P.stride,
                       d_q, (int64_t)1);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error("vector update pair launch", e);
    (void)hipStreamSynchronize(s);
    if (block) dot_block_give(block, s, false);
    return SPL_ERROR_device;
  }
  if (block) dot_block_give(block, s, true);
  return SPL_OK;
}

}  // namespace spl

// umfpack_zi.hip — the complex (`zi`) half of the UMFPACK link-time ABI
// (suitesparse/src/Numeric/LinearAlgebra/Umfpack/Internal.hs:69-135).
//
// Round 3: where the analysis chooses the multifrontal tree (and the tree has work to halve), the factors are NATIVE
// COMPLEX fronts on the tree of the complex pattern (csrc/multifrontal.hip, TreeView::zm; csrc/dense_lu_kernels.hpp,
// the *_z functions).  The object still holds the real embedding described below — packed complex vectors are its
// real vectors, so the complex factors solve it — for residuals, refinement and every fallback; the band path and
// small trees factor it as before.
//
// A complex n x n system  (R + iI)(x + iy) = b + ic  is solved as the real 2n x 2n system with
// interleaved unknowns (x0, y0, x1, y1, ...):  block (i,j) of the embedding E is [[R, -I], [I, R]].
// Packed complex vectors (the only form the reference uses: Az = Xz = Bz = NULL,
// Internal.hs:124-132) are then exactly the real vectors of the embedded system, and E^T is the
// embedding of A^H, so sys = 1 (UMFPACK_At, the conjugate transpose) maps to the real transposed
// solve.  Symbolic / Numeric handles are the `di` handles of E; all arithmetic runs in the same
// GPU kernels as the real path (band LU, banded solves, SpMV-based refinement); values differ from a complex-
// arithmetic LU only in rounding, and `ident <\> v == v` (suitesparse/tests/test-umfpack.hs:16-19,
// on Vector (Complex Double)) holds exactly.
//
// Complex SYMMETRIC matrices (A == A^T, not Hermitian: FEAST's z B - A for real symmetric A, B) get a SYMMETRIC real
// embedding, so that the multifrontal tree runs in its L D L^T mode (half the flops, dense_lu_kernels.hpp Band::sym):
// with M(a) = [[re a, -im a], [im a, re a]] and C = diag(1, -1), the block C M(w) = [[re w, -im w], [-im w, -re w]]
// is a symmetric 2 x 2 matrix for every complex w, hence E' = (C M(w_ij)) is symmetric whenever w_ij = w_ji.  w is
// A under the congruence D A D with a unit-modulus diagonal D = diag(u_r), u_r^2 = conj(a_rr) / |a_rr|: the diagonal
// of D A D is real and positive, so the scalar pivots of a diagonal block start as +|a_rr|, -|a_rr| (the role the
// swap of the two equations plays in the general case).  E' = T E W with T = blockdiag(C M(u_r)), W =
// blockdiag(M(u_r)):  A x = b  is  E' x' = T b, x = W x';  A^H y = c  is  E' y' = W^T c, y = T^T y'.
#include <chrono>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <cstdio>
#include <memory>
#include <thread>
#include <utility>
#include <vector>

#include "umfpack_impl.hpp"

namespace {

// CSC arrays of the embedding E (2n x 2n, 4 entries per complex entry, rows ascending)
struct Embedded {
  // plain arrays, NOT std::vector: resize() would zero 240 MB on one thread (40 ms at 10^6 unknowns) before the
  // threads of embed() write every element anyway
  template <typename T>
  struct Raw {
    std::unique_ptr<T[]> mem;
    void resize(size_t n) { mem.reset(new T[n ? n : 1]); }
    T *data() const { return mem.get(); }
    T &operator[](size_t k) const { return mem[k]; }
  };
  Raw<int> p, i;
  Raw<double> x;
};

// swap[r] != 0: the two real rows of complex row r change places (static pivoting, see numeric)
// unit != nullptr: the symmetric embedding C M(u_r a_rj u_j) of a complex symmetric matrix (see the head of this file)
bool embed(int n, const int *Ap, const int *Ai, const double *Ax, const double *Az, bool values, Embedded &E,
           const char *swap = nullptr, const double *unit = nullptr) {
  const long nnz = Ap[n];
  if (4 * nnz >= 0x7fffffffL) return false;
  E.p.resize((size_t)2 * n + 1);
  E.i.resize((size_t)4 * nnz);
  if (values) E.x.resize((size_t)4 * nnz);
  // column 2j starts at 4 Ap[j], column 2j + 1 one block column (2 entries per stored entry) further: no running
  // counter, so the columns are shared out among threads (20 million entries at 10^6 unknowns: 48 ms on one core,
  // a third of a FEAST-style refactorisation)
  auto fill = [&](int j0, int j1) {
    for (int j = j0; j < j1; ++j) {
      const long len = Ap[j + 1] - Ap[j];
      for (int half = 0; half < 2; ++half) {
        long q = 4 * (long)Ap[j] + 2 * len * half;
        E.p[(size_t)2 * j + half] = (int)q;
        for (int p = Ap[j]; p < Ap[j + 1]; ++p) {
          const int r = Ai[p];
          E.i[(size_t)q] = 2 * r;
          E.i[(size_t)q + 1] = 2 * r + 1;
          if (values) {
            const double re = Az ? Ax[p] : Ax[2 * (size_t)p];
            const double im = Az ? Az[p] : Ax[2 * (size_t)p + 1];
            if (unit) {
              // w = (u_lo u_hi) a with the two units taken in index order: entries (r, j) and (j, r) of a symmetric
              // matrix go through the same operations on the same operands and get the same bits
              const int lo = r < j ? r : j, hi = r < j ? j : r;
              const double ar = unit[2 * (size_t)lo], ai = unit[2 * (size_t)lo + 1];
              const double br = unit[2 * (size_t)hi], bi = unit[2 * (size_t)hi + 1];
              const double pr = ar * br - ai * bi, pi = ar * bi + ai * br;
              const double wr = pr * re - pi * im, wi = pr * im + pi * re;
              E.x[(size_t)q] = half == 0 ? wr : -wi;
              E.x[(size_t)q + 1] = half == 0 ? -wi : -wr;
              q += 2;
              continue;
            }
            const double top = half == 0 ? re : -im, bottom = half == 0 ? im : re;
            const bool sw = swap && swap[r];
            E.x[(size_t)q] = sw ? bottom : top;
            E.x[(size_t)q + 1] = sw ? top : bottom;
          }
          q += 2;
        }
      }
    }
  };
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt ? (nt > 8 ? 8 : nt) : 1;
  if (nnz < 200000 || nt < 2) {
    fill(0, n);
  } else {
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nt; ++t) {
      const int j0 = (int)((long)n * t / nt), j1 = (int)((long)n * (t + 1) / nt);
      try {
        pool.emplace_back(fill, j0, j1);
      } catch (...) {  // a thread could not be started: its columns are done here
        fill(j0, j1);
      }
    }
    fill(0, (int)((long)n / nt));
    for (std::thread &th : pool) th.join();
  }
  E.p[(size_t)2 * n] = (int)(4 * nnz);
  return true;
}

// v <- Q v: the entries 2r, 2r+1 of a packed complex vector change places where swap[r] is set
void swap_pairs(const std::vector<char> &swap, double *v) {
  for (size_t r = 0; r < swap.size(); ++r)
    if (swap[r]) std::swap(v[2 * r], v[2 * r + 1]);
}

// device form of swap_pairs: one thread per complex entry of n x k packed vectors
__global__ __launch_bounds__(256) void swap_pairs_kernel(const char *__restrict__ flags, double *__restrict__ v,
                                                         size_t n, size_t total) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total || !flags[t % n]) return;
  const double a = v[2 * t], b = v[2 * t + 1];
  v[2 * t] = b;
  v[2 * t + 1] = a;
}

// A == A^T exactly (pattern and bits of the values)?  Every off-diagonal entry looks its partner up by bisection.
bool complex_symmetric(int n, const int *Ap, const int *Ai, const double *Ax, const double *Az) {
  std::atomic<bool> ok{true};
  auto same = [&](int p, int q) {
    if (Az) return std::memcmp(&Ax[p], &Ax[q], sizeof(double)) == 0 && std::memcmp(&Az[p], &Az[q], sizeof(double)) == 0;
    return std::memcmp(&Ax[2 * (size_t)p], &Ax[2 * (size_t)q], 2 * sizeof(double)) == 0;
  };
  auto check = [&](int j0, int j1) {
    for (int j = j0; j < j1; ++j) {
      if (!ok.load(std::memory_order_relaxed)) return;
      for (int p = Ap[j]; p < Ap[j + 1]; ++p) {
        const int r = Ai[p];
        if (r == j) continue;
        const int *first = Ai + Ap[r], *last = Ai + Ap[r + 1];
        const int *it = std::lower_bound(first, last, j);
        if (it == last || *it != j || !same(p, (int)(it - Ai))) {
          ok.store(false, std::memory_order_relaxed);
          return;
        }
      }
    }
  };
  unsigned nt = std::thread::hardware_concurrency();
  nt = nt ? (nt > 8 ? 8 : nt) : 1;
  if (Ap[n] < 200000 || nt < 2) {
    check(0, n);
  } else {
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nt; ++t) {
      const int j0 = (int)((long)n * t / nt), j1 = (int)((long)n * (t + 1) / nt);
      try {
        pool.emplace_back(check, j0, j1);
      } catch (...) {
        check(j0, j1);
      }
    }
    check(0, (int)((long)n / nt));
    for (std::thread &th : pool) th.join();
  }
  return ok.load();
}

// The 2 x 2 transforms of the symmetric embedding on a packed complex vector v of n entries (u: n unit-modulus pairs):
//   0: v <- C (u v)   right-hand side of A x = b         1: v <- u v              its solution
//   2: v <- conj(u) v right-hand side of A^H y = c       3: v <- conj(u) conj(v)  its solution
__host__ __device__ inline void unit_pair(int mode, double ur, double ui, double &vr, double &vi) {
  if (mode >= 2) ui = -ui;
  const double xr = vr, xi = mode == 3 ? -vi : vi;
  const double tr = ur * xr - ui * xi, ti = ur * xi + ui * xr;
  vr = tr;
  vi = mode == 0 ? -ti : ti;
}
void unit_pairs(const std::vector<double> &u, int mode, double *v) {
  for (size_t r = 0; r < u.size() / 2; ++r) unit_pair(mode, u[2 * r], u[2 * r + 1], v[2 * r], v[2 * r + 1]);
}
__global__ __launch_bounds__(256) void unit_pairs_kernel(const double *__restrict__ u, int mode, double *__restrict__ v,
                                                         size_t n, size_t total) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const size_t r = t % n;
  double vr = v[2 * t], vi = v[2 * t + 1];
  unit_pair(mode, u[2 * r], u[2 * r + 1], vr, vi);
  v[2 * t] = vr;
  v[2 * t + 1] = vi;
}

struct ZiSymbolic {  // remembers n so that numeric can rebuild the embedding, and the complex pattern it analysed
  unsigned magic = 0x5A53594Du;
  int n = 0;
  spl::Symbolic *di = nullptr;
  std::vector<int> Ap;
  uint64_t ai_hash = 0;
  spl::DevicePattern dpat;  // the complex pattern in a handle's layout (the numeric calls on handles)
};

// What umfpack_zi_numeric decides before it embeds — the same decisions for host arrays and for a handle; only where
// the symmetry test runs differs (`symmetric_matrix` is asked at most once).
struct ZiChoice {
  bool native = false;     // native complex fronts take the plain embedding
  bool is_sym = false;     // A == A^T was wanted and holds
  bool symmetric = false;  // the symmetric congruence embedding
};

// Native complex fronts serve this analysis?  They need the tree (of the complex pattern), and pay where the tree has
// flops to halve: below ~1e12 flops of the embedding's tree (2-D meshes up to 10^6 unknowns) a factorisation is
// launch-bound either way and a batch of right-hand sides takes twice the passes over the tree (four complex columns
// per pass against eight real ones).  SPL_ZI_NATIVE=1 / 0: always / never.
bool native_fronts(const spl::Symbolic &S) {
  if (!S.tree || !S.ztree) return false;
  const char *zn = getenv("SPL_ZI_NATIVE");
  if (zn && zn[0] == '0') return false;
  if (zn && zn[0] == '1') return true;
  return S.tree->flops >= 1e12;
}

template <typename SymmetryTest>
ZiChoice zi_choice(const spl::Symbolic &S, int n, SymmetryTest &&symmetric_matrix) {
  ZiChoice c;
  c.native = native_fronts(S);
  const char *zs = getenv("SPL_ZI_SYMMETRIC");
  const bool wanted = c.native || (zs ? zs[0] != '0' : (S.tree ? S.tree->flops : 0.0) >= 1e12);
  c.is_sym = wanted && n > 1 && symmetric_matrix();
  c.symmetric = c.is_sym && !c.native;
  return c;
}

// What the `zi` calls on handles ask of H before anything else: a whole complex matrix with 32-bit row pointers
// (UMFPACK_ERROR_invalid_matrix) whose real embedding, four entries per stored entry, stays below 2^31 entries when it
// is square (UMFPACK_ERROR_out_of_memory, as embed() reports; a rectangular matrix is never embedded).  The size is a
// property of the handle alone, so it is refused here, before the pattern is exported or compared.
int zi_handle_status(const spl::Matrix *M) {
  const int hs = spl::handle_status(M, 2);
  if (hs != UMFPACK_OK) return hs;
  if (M->nrows_global == M->ncols && 4 * M->nnz >= 0x7fffffffLL) return UMFPACK_ERROR_out_of_memory;
  return UMFPACK_OK;
}

// the line SPL_MF_TIMING prints about the embedding
void report_embedding(const ZiChoice &c, const char *where, std::chrono::steady_clock::time_point t0) {
  fprintf(stderr, "[zi numeric] %s embedding built on the %s %8.2f ms\n",
          c.native ? (c.is_sym ? "plain (native complex fronts, symmetric)" : "plain (native complex fronts)")
                   : c.symmetric ? "symmetric" : "general",
          where, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// nrhs complex systems on the host through the real embedding N holds: right-hand sides packed (re, im) pairs when
// the imaginary pointers are NULL, else split arrays of n x nrhs (column-major); interleave, apply the swapped pairs
// and the congruence, solve, undo both, de-interleave
int solve_host(spl::Numeric *N, int sys, const int *Ap, const int *Ai, const double *Ax, int nrhs, double *Xx,
               double *Xz, const double *Bx, const double *Bz, double *Info) {
  return spl::umf_guarded([&] {
    const std::vector<char> &swap = N->pair_swap;
    const std::vector<double> &unit = N->pair_unit;
    const size_t n2 = (size_t)N->n, n = n2 / 2, tot = n2 * (size_t)nrhs;
    const bool packed = !Xz && !Bz;
    std::vector<double> b(tot), x(tot);
    for (size_t c = 0; c < (size_t)nrhs; ++c) {
      for (size_t k = 0; k < n; ++k) {
        b[c * n2 + 2 * k] = packed ? Bx[c * n2 + 2 * k] : Bx[c * n + k];
        b[c * n2 + 2 * k + 1] = packed ? Bx[c * n2 + 2 * k + 1] : (Bz ? Bz[c * n + k] : 0.0);
      }
      if (!swap.empty() && sys == UMFPACK_A) swap_pairs(swap, b.data() + c * n2);     // (Q E) x = Q b
      if (!unit.empty()) unit_pairs(unit, sys == UMFPACK_A ? 0 : 2, b.data() + c * n2);  // E' x' = T b  /  E' y' = W^T c
    }
    const int st = sys != UMFPACK_A && sys != UMFPACK_At
                       ? UMFPACK_ERROR_invalid_system
                       : spl::solve_columns(N, sys, nrhs, x.data(), b.data(), Ap, Ai, Ax, false, Info);
    for (size_t c = 0; c < (size_t)nrhs; ++c) {
      if (!swap.empty() && sys != UMFPACK_A) swap_pairs(swap, x.data() + c * n2);       // y = Q w
      if (!unit.empty()) unit_pairs(unit, sys == UMFPACK_A ? 1 : 3, x.data() + c * n2);  // x = W x'  /  y = T^T y'
      for (size_t k = 0; k < n; ++k) {
        if (packed) { Xx[c * n2 + 2 * k] = x[c * n2 + 2 * k]; Xx[c * n2 + 2 * k + 1] = x[c * n2 + 2 * k + 1]; }
        else { Xx[c * n + k] = x[c * n2 + 2 * k]; if (Xz) Xz[c * n + k] = x[c * n2 + 2 * k + 1]; }
      }
    }
    return st;
  });
}

// nrhs packed complex systems in device memory through the real embedding N holds: apply the swapped pairs or the unit
// congruence to the right-hand sides, solve_embedded(b) the embedded systems into d_X, undo them on the solutions
template <typename Solve>
int solve_dev(spl::Numeric *N, int sys, int nrhs, double *d_X, const double *d_B, Solve &&solve_embedded) {
  const std::vector<char> *swap = !N->pair_swap.empty() ? &N->pair_swap : nullptr;
  const std::vector<double> *unit = !N->pair_unit.empty() ? &N->pair_unit : nullptr;
  if ((!swap && !unit) || nrhs == 0 || N->n == 0) return solve_embedded(d_B);
  if (sys != UMFPACK_A && sys != UMFPACK_At) return UMFPACK_ERROR_invalid_system;
  return spl::umf_guarded([&] {
    const size_t n = (size_t)N->n / 2, total = n * (size_t)nrhs;
    if (unit) {  // symmetric embedding: E' x' = T b, x = W x'  /  E' y' = W^T c, y = T^T y'
      spl::DBuf<double> u(2 * n), b(2 * total);
      SPL_HIP(hipMemcpy(u.get(), unit->data(), 2 * n * sizeof(double), hipMemcpyHostToDevice));
      SPL_HIP(hipMemcpy(b.get(), d_B, 2 * total * sizeof(double), hipMemcpyDeviceToDevice));
      const dim3 grid((unsigned)((total + 255) / 256));
      hipLaunchKernelGGL(unit_pairs_kernel, grid, dim3(256), 0, nullptr, u.get(), sys == UMFPACK_A ? 0 : 2, b.get(), n, total);
      SPL_HIP(hipDeviceSynchronize());
      const int st = solve_embedded(b.get());
      if (st < 0) return st;
      hipLaunchKernelGGL(unit_pairs_kernel, grid, dim3(256), 0, nullptr, u.get(), sys == UMFPACK_A ? 1 : 3, d_X, n, total);
      SPL_HIP(hipDeviceSynchronize());
      return st;
    }
    spl::DBuf<char> flags(n);
    SPL_HIP(hipMemcpy(flags.get(), swap->data(), n, hipMemcpyHostToDevice));
    const dim3 grid((unsigned)((total + 255) / 256));
    if (sys == UMFPACK_A) {  // (Q E) x = Q b
      spl::DBuf<double> b(2 * total);
      SPL_HIP(hipMemcpy(b.get(), d_B, 2 * total * sizeof(double), hipMemcpyDeviceToDevice));
      hipLaunchKernelGGL(swap_pairs_kernel, grid, dim3(256), 0, nullptr, flags.get(), b.get(), n, total);
      SPL_HIP(hipDeviceSynchronize());
      return solve_embedded(b.get());
    }
    const int st = solve_embedded(d_B);
    if (st < 0) return st;
    hipLaunchKernelGGL(swap_pairs_kernel, grid, dim3(256), 0, nullptr, flags.get(), d_X, n, total);  // y = Q w
    SPL_HIP(hipDeviceSynchronize());
    return st;
  });
}

}  // namespace

extern "C" {

int umfpack_zi_symbolic(int n_row, int n_col, const int Ap[], const int Ai[], const double Ax[],
                        const double Az[], void **SymbolicOut, const double Control[], double Info[]) {
  (void)Ax; (void)Az; (void)Control; (void)Info;
  if (!SymbolicOut) return UMFPACK_ERROR_argument_missing;
  *SymbolicOut = nullptr;
  if (!Ap) return UMFPACK_ERROR_argument_missing;
  if (n_row <= 0 || n_col <= 0) return UMFPACK_ERROR_n_nonpositive;
  // (a missing Ai is an invalid matrix here, a missing argument for umfpack_di_symbolic)
  if (Ap[0] != 0 || Ap[n_col] < 0 || (Ap[n_col] > 0 && !Ai)) return UMFPACK_ERROR_invalid_matrix;
  const int valid = spl::validate_host_csc(n_row, n_col, Ap, Ai);
  if (valid != UMFPACK_OK) return valid;
  return spl::umf_guarded([&] {
    std::unique_ptr<ZiSymbolic> S(new ZiSymbolic());
    S->n = n_col;
    int st;
    if (n_row != n_col) {  // rectangular: shape and pattern only (umfpack.hip, Symbolic::rectangular)
      st = spl::symbolic_rectangular(n_row, n_col, Ap, Ai, &S->di);
    } else {
      Embedded E;
      if (!embed(n_col, Ap, Ai, nullptr, nullptr, false, E)) return UMFPACK_ERROR_out_of_memory;
      S->Ap.assign(Ap, Ap + n_col + 1);
      S->ai_hash = spl::hash_indices(Ai, Ap[n_col]);
      // ordered on the complex pattern (half the vertices, a quarter of the edges of the embedding), then expanded
      st = spl::symbolic_common(n_col, Ap, Ai, 2, E.p.data(), E.i.data(), &S->di);
    }
    if (st >= 0) *SymbolicOut = S.release();
    return st;
  });
}

int umfpack_zi_numeric(const int Ap[], const int Ai[], const double Ax[], const double Az[],
                       void *SymbolicIn, void **NumericOut, const double Control[], double Info[]) {
  (void)Control; (void)Info;
  if (!NumericOut) return UMFPACK_ERROR_argument_missing;
  *NumericOut = nullptr;
  ZiSymbolic *S = static_cast<ZiSymbolic *>(SymbolicIn);
  if (!S || S->magic != 0x5A53594Du) return UMFPACK_ERROR_invalid_Symbolic_object;
  if (!Ap || !Ai || !Ax) return UMFPACK_ERROR_argument_missing;
  spl::Numeric *N = nullptr;
  const int st = spl::umf_guarded([&] {
    if (S->di->rectangular) {
      const int nnz = Ap[S->n];
      if (nnz < 0) return UMFPACK_ERROR_different_pattern;
      std::vector<char> nonzero((size_t)nnz);
      for (int p = 0; p < nnz; ++p) {
        const double re = Az ? Ax[p] : Ax[2 * (size_t)p], im = Az ? Az[p] : Ax[2 * (size_t)p + 1];
        nonzero[(size_t)p] = ((re != 0.0 || im != 0.0) && re == re && im == im) ? 1 : 0;
      }
      return spl::numeric_rectangular(S->di, Ap, Ai, nonzero, &N, Ax, Az ? Az : Ax + 1, Az ? 1 : 2);
    }
    // Static pivoting inside the 2 x 2 blocks of the diagonal.  The scalar factorisation of the
    // embedding pivots on the REAL part of a complex diagonal entry first; where the imaginary part
    // is the larger one (a shift z I - A close to the real axis of A's diagonal: pivot ~ 0), the two
    // real equations of that complex row change places, so that the first pivot is the imaginary
    // part.  A row permutation Q of the system: (Q E) x = Q b; E^T y = c is (Q E)^T (Q y) = c.  The
    // pattern of the embedding does not change (every block is a full 2 x 2).
    const int n = S->n;
    // UMFPACK_ERROR_different_pattern, decided on the complex pattern (the embedding's is four times as long)
    if (!std::equal(S->Ap.begin(), S->Ap.end(), Ap) || spl::hash_indices(Ai, Ap[n]) != S->ai_hash)
      return UMFPACK_ERROR_different_pattern;
    const bool timing = getenv("SPL_MF_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    // A complex symmetric matrix (FEAST's z B - A for real symmetric A, B) is embedded symmetrically and factored as
    // L D L^T (head of this file) where the tree has work to halve: below ~1e12 flops (2-D meshes of 10^6 unknowns, 3-D ones below ~50^3) the
    // factorisation is launch-bound and the symmetry check on the host costs more than the flops saved.
    // SPL_ZI_SYMMETRIC=0: the general embedding for every matrix; =1: the symmetric one whenever A == A^T
    // Native complex fronts (csrc/multifrontal.hip, TreeView::zm) take the PLAIN embedding — no swapped pairs, no
    // congruence: a complex pivot is as good as its modulus — whenever the analysis chose the tree; a complex symmetric
    // matrix is then factored as L D L^T in complex arithmetic.  The embeddings below serve the band path, and
    // SPL_ZI_NATIVE=0.
    const ZiChoice choice = zi_choice(*S->di, n, [&] { return complex_symmetric(n, Ap, Ai, Ax, Az); });
    const bool native = choice.native, is_sym = choice.is_sym, symmetric = choice.symmetric;
    std::vector<char> swap;
    std::vector<double> unit;
    bool any = false;
    if (symmetric) {
      unit.assign((size_t)2 * n, 0.0);
      for (int j = 0; j < n; ++j) {
        unit[(size_t)2 * j] = 1.0;
        const int *first = Ai + Ap[j], *last = Ai + Ap[j + 1];
        const int *it = std::lower_bound(first, last, j);
        if (it == last || *it != j) continue;
        const size_t p = (size_t)(it - Ai);
        const double re = Az ? Ax[p] : Ax[2 * p], im = Az ? Az[p] : Ax[2 * p + 1];
        spl::congruence_unit(re, im, &unit[(size_t)2 * j]);
      }
    } else if (!native) {
      swap.assign((size_t)n, 0);
      for (int j = 0; j < n; ++j)
        for (int p = Ap[j]; p < Ap[j + 1]; ++p)
          if (Ai[p] == j) {
            const double re = Az ? Ax[p] : Ax[2 * (size_t)p], im = Az ? Az[p] : Ax[2 * (size_t)p + 1];
            if (std::fabs(im) > std::fabs(re)) { swap[(size_t)j] = 1; any = true; }
          }
    }
    Embedded E;
    if (!embed(n, Ap, Ai, Ax, Az, true, E, any ? swap.data() : nullptr, symmetric ? unit.data() : nullptr))
      return UMFPACK_ERROR_out_of_memory;
    if (timing) report_embedding(choice, "host", t0);
    spl::EmbeddingOpts opts;
    opts.embedding = true;
    opts.native = native;
    opts.zsym = native && is_sym;
    if (any) opts.pair_swap = std::move(swap);
    if (symmetric) opts.pair_unit = std::move(unit);
    return spl::numeric_factor(S->di, E.p.data(), E.i.data(), E.x.data(), std::move(opts), &N);
  });
  *NumericOut = N;
  return st;
}

// ---- the same two calls on a device-resident complex matrix handle (umfpack_hip.h; kernels in lu_from_handle.hip) ---

int spl_umfpack_zi_symbolic_dev(void *H, void **SymbolicOut) {
  if (!SymbolicOut) return UMFPACK_ERROR_argument_missing;
  *SymbolicOut = nullptr;
  spl::Matrix *M = spl::as_matrix(H);
  if (!M) return UMFPACK_ERROR_argument_missing;
  const int hs = zi_handle_status(M);
  if (hs != UMFPACK_OK) return hs;
  return spl::umf_guarded([&] {
    spl::DeviceGuard g(M->device);
    // the analysis is host code: the pattern crosses once, here
    std::vector<int> Ap, Ai;
    spl::handle_to_host_csc(M, Ap, Ai, nullptr);
    void *S = nullptr;
    const int st = umfpack_zi_symbolic((int)M->nrows_global, (int)M->ncols, Ap.data(), Ai.data(), nullptr, nullptr, &S,
                                       nullptr, nullptr);
    if (st < 0) return st;
    try {
      spl::pattern_from_handle(M, static_cast<ZiSymbolic *>(S)->dpat, hipStreamPerThread);
    } catch (...) {
      umfpack_zi_free_symbolic(&S);
      throw;
    }
    *SymbolicOut = S;
    return st;
  });
}

int spl_umfpack_zi_numeric_dev(void *H, void *SymbolicIn, void **NumericOut) {
  if (!NumericOut) return UMFPACK_ERROR_argument_missing;
  *NumericOut = nullptr;
  ZiSymbolic *S = static_cast<ZiSymbolic *>(SymbolicIn);
  if (!S || S->magic != 0x5A53594Du) return UMFPACK_ERROR_invalid_Symbolic_object;
  spl::Matrix *M = spl::as_matrix(H);
  if (!M) return UMFPACK_ERROR_argument_missing;
  const int hs = zi_handle_status(M);
  if (hs != UMFPACK_OK) return hs;
  spl::Numeric *N = nullptr;
  const int st = spl::umf_guarded([&] {
    spl::DeviceGuard g(M->device);
    if (S->di->rectangular) {  // no factors are kept: the host route, with its statuses
      if (M->nrows_global != S->di->n_row || M->ncols != S->di->n_col) return UMFPACK_ERROR_different_pattern;
      std::vector<int> Ap, Ai;
      std::vector<double> Ax;
      spl::handle_to_host_csc(M, Ap, Ai, &Ax);
      void *out = nullptr;
      const int sr = umfpack_zi_numeric(Ap.data(), Ai.data(), Ax.data(), nullptr, S, &out, nullptr, nullptr);
      N = static_cast<spl::Numeric *>(out);
      return sr;
    }
    const int n = S->n;
    hipStream_t s = hipStreamPerThread;
    if (M->nrows_global != n || M->ncols != n || M->nnz != (int64_t)S->Ap[(size_t)n] ||
        !spl::handle_has_pattern(M, S->dpat, S->Ap, S->ai_hash, s))
      return UMFPACK_ERROR_different_pattern;
    const bool timing = getenv("SPL_MF_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    // the decisions of umfpack_zi_numeric, their inputs computed where the matrix is: symmetry, swap flags and units
    // by kernels over the handle's image; n bytes of flags or 16 n of units come down for the solves
    const ZiChoice choice = zi_choice(*S->di, n, [&] { return spl::complex_handle_symmetric(M, s); });
    spl::ComplexDiagonal D;
    if (choice.symmetric) spl::complex_handle_diagonal(M, true, D, s);
    else if (!choice.native) spl::complex_handle_diagonal(M, false, D, s);
    spl::EmbeddingOpts opts;
    opts.embedding = true;
    opts.native = choice.native;
    opts.zsym = choice.native && choice.is_sym;
    if (D.any_swap) opts.pair_swap = std::move(D.swap);
    if (choice.symmetric) opts.pair_unit = std::move(D.unit);
    // rows of E: the embedding kernel; rows of E^T: its transpose on the device (exact and order-preserving: the two
    // images are those the host route makes from embed()'s CSC arrays)
    const spl::StageImages from_handle = [&](spl::Numeric *Nn, hipStream_t ss, const std::function<void(const char *)> &lap) {
      Nn->A = spl::embed_handle(M, D.any_swap ? D.d_swap.get() : nullptr, choice.symmetric ? D.d_unit.get() : nullptr, ss);
      if (!Nn->A->rowptr.get()) return UMFPACK_ERROR_out_of_memory;
      if (timing) report_embedding(choice, "device", t0);
      lap("rows of E (embedding)");
      return spl::stage_transposed_image(Nn, true);
    };
    return spl::numeric_factor_staged(S->di, std::move(opts), from_handle, nullptr, nullptr, nullptr, &N);
  });
  *NumericOut = N;
  return st;
}

int umfpack_zi_solve(int sys, const int Ap[], const int Ai[], const double Ax[], const double Az[],
                     double Xx[], double Xz[], const double Bx[], const double Bz[], void *NumericIn,
                     const double Control[], double Info[]) {
  (void)Az;
  spl::Numeric *N = spl::as_numeric(NumericIn);
  const int st = [&] {
    if (N && N->rectangular) return UMFPACK_ERROR_invalid_system;
    if (!Xx || !Bx) return UMFPACK_ERROR_argument_missing;
    if (!Ap || !Ai || !Ax) return UMFPACK_ERROR_argument_missing;
    if (!N) return UMFPACK_ERROR_invalid_Numeric_object;
    // the Numeric object holds device copies of E and E^T (residuals use those, like the `di` path)
    if (!Xz && !Bz && N->pair_swap.empty() && N->pair_unit.empty())
      return umfpack_di_solve(sys, Ap, Ai, Ax, Xx, Bx, NumericIn, Control, Info);
    return solve_host(N, sys, Ap, Ai, Ax, 1, Xx, Xz, Bx, Bz, Info);
  }();
  if (Info && st < 0) Info[0] = st;  // Info[UMFPACK_STATUS] on the error returns as well
  return st;
}

// batched complex linearSolve: nrhs right-hand sides, each packed (re, im) pairs when the
// imaginary pointers are NULL, else split arrays of n x nrhs (column-major)
int spl_umfpack_zi_solve_many(int sys, const int Ap[], const int Ai[], const double Ax[], const double Az[],
                              int nrhs, double Xx[], double Xz[], const double Bx[], const double Bz[],
                              void *NumericIn) {
  (void)Az;
  spl::Numeric *N = spl::as_numeric(NumericIn);
  if (N && N->rectangular) return UMFPACK_ERROR_invalid_system;
  if (nrhs < 0) return UMFPACK_ERROR_argument_missing;
  if (!Ap || !Ai || !Ax) return UMFPACK_ERROR_argument_missing;
  if (!N) return UMFPACK_ERROR_invalid_Numeric_object;
  if (nrhs > 0 && N->n > 0 && (!Xx || !Bx)) return UMFPACK_ERROR_argument_missing;
  if (!Xz && !Bz && N->pair_swap.empty() && N->pair_unit.empty())
    return spl_umfpack_di_solve_many(sys, Ap, Ai, Ax, nrhs, Xx, Bx, NumericIn);
  return solve_host(N, sys, Ap, Ai, Ax, nrhs, Xx, Xz, Bx, Bz, nullptr);
}

// packed complex right-hand sides and solutions in device memory (see umfpack_hip.h)
int spl_umfpack_zi_solve_many_dev(int sys, const int Ap[], const int Ai[], const double Ax[], int nrhs, double *d_X,
                                  const double *d_B, void *NumericIn) {
  spl::Numeric *N = spl::as_numeric(NumericIn);
  if (N && N->rectangular) return UMFPACK_ERROR_invalid_system;
  if (nrhs < 0) return UMFPACK_ERROR_argument_missing;
  const int n2 = N ? N->n : 0;
  if (n2 == 0 && !NumericIn) return UMFPACK_ERROR_invalid_Numeric_object;
  if (nrhs > 0 && n2 > 0 && (!d_X || !d_B)) return UMFPACK_ERROR_argument_missing;
  const bool plain = !N || (N->pair_swap.empty() && N->pair_unit.empty());
  if (plain || nrhs == 0 || n2 == 0) return spl_umfpack_di_solve_many_dev(sys, Ap, Ai, Ax, nrhs, d_X, d_B, NumericIn);
  return solve_dev(N, sys, nrhs, d_X, d_B, [&](const double *b) {
    return spl_umfpack_di_solve_many_dev(sys, Ap, Ai, Ax, nrhs, d_X, b, NumericIn);
  });
}

// kappa_1(A) / kappa_1(A^H) = kappa_inf(A) of a complex matrix: the estimator's solves are those of
// spl_umfpack_zi_solve_many_dev, with the object's turn held (umfpack.hip: condest_numeric)
int spl_umfpack_zi_condest(int sys, int t, const int Ap[], const int Ai[], const double Ax[], const double Az[],
                           void *NumericIn, double out[6], double xx[], double xz[]) {
  (void)Az;
  if (out)
    for (int i = 0; i < 6; ++i) out[i] = 0.0;
  spl::Numeric *N = spl::as_numeric(NumericIn);
  const int st = spl::condest_arguments(N, true, sys, t, out, Ap, Ai, Ax);
  if (st != UMFPACK_OK) return st;
  const spl::DeviceSolve solve = [N](int sys_c, int k, double *d_X, const double *d_B) {
    return solve_dev(N, sys_c, k, d_X, d_B, [&](const double *b) {
      return spl::solve_columns(N, sys_c, k, d_X, b, nullptr, nullptr, nullptr, true, nullptr, true);
    });
  };
  std::vector<double> w(xx ? (size_t)N->n : 0);
  const int cst = spl::condest_numeric(N, sys, t, 2, solve, out, xx ? w.data() : nullptr);
  if (cst == UMFPACK_OK && xx) {
    const size_t n = (size_t)N->n / 2;
    for (size_t k = 0; k < n; ++k) {
      if (xz) { xx[k] = w[2 * k]; xz[k] = w[2 * k + 1]; }
      else { xx[2 * k] = w[2 * k]; xx[2 * k + 1] = w[2 * k + 1]; }
    }
  }
  return cst;
}

void umfpack_zi_free_symbolic(void **Symbolic) {
  if (!Symbolic || !*Symbolic) return;
  ZiSymbolic *S = static_cast<ZiSymbolic *>(*Symbolic);
  *Symbolic = nullptr;
  if (S->magic != 0x5A53594Du) return;
  S->magic = 0;
  void *di = S->di;
  umfpack_di_free_symbolic(&di);
  delete S;
}

void umfpack_zi_free_numeric(void **Numeric) { umfpack_di_free_numeric(Numeric); }

void umfpack_zi_report_status(const double Control[], int status) { umfpack_di_report_status(Control, status); }

}  // extern "C"

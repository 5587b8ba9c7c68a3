// umfpack_impl.hpp — the objects behind the UMFPACK handles and the internal calls between the real (`di`,
// umfpack.hip) and the complex (`zi`, umfpack_zi.hip) halves of the ABI.  Included by those two files and by
// lu_from_handle.hip (what their calls on device-resident handles run on the device) only.
#pragma once
#include <atomic>
#include <cmath>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "common.hpp"
#include "mf_symbolic.hpp"
#include "../../include/umfpack_hip.h"

namespace spl {

constexpr uint32_t kSymMagic = 0x53594D42u;  // "SYMB"
constexpr uint32_t kNumMagic = 0x4E554D52u;  // "NUMR"

// The analysed pattern on the device, in the layout of a matrix handle (row pointers and column indices of the rows
// image): what the numeric calls on handles compare against (lu_from_handle.hip).  Made by the analysis of a handle, or
// by the first numeric call on a handle with a host-born analysis (under `mu`: several threads factor with one
// Symbolic).
struct DevicePattern {
  std::mutex mu;
  std::atomic<bool> ready{false};
  int64_t nrows = 0, nnz = 0;
  DBuf<int> rowptr, colidx;
};

struct Symbolic {
  uint32_t magic = kSymMagic;
  DevicePattern dpat;
  int n = 0;
  int nnz = 0;
  int kl = 0, ku = 0;
  std::vector<int> perm;  // new -> old (reverse Cuthill-McKee: the band paths)
  std::vector<int> inv;   // old -> new
  std::vector<int> Ap;    // pattern check in numeric (UMFPACK_ERROR_different_pattern)
  uint64_t ai_hash = 0;   // ... together with a hash of the row indices
  // nested-dissection tree of the multifrontal path, present when that path is the cheaper one
  std::shared_ptr<const mf::Tree> tree;
  // embeddings of complex matrices (umfpack_zi.hip): the tree of the COMPLEX pattern itself, from the same dissection
  // (tree is its expansion): what the native complex fronts are built on
  std::shared_ptr<const mf::Tree> ztree;
  bool have_band = false;  // perm / inv / kl / ku are set (large matrices whose tree wins by a lower bound skip them)
  // Rectangular matrices (round 4).  UMFPACK analyses and factors them and refuses to SOLVE with them
  // (UMFPACK_ERROR_invalid_system: "the matrix is not square"); through the reference's binding nothing of such a
  // factorisation is observable but the statuses (Umfpack.hs:60-102 binds symbolic, numeric, solve and the frees).
  // Here: the analysis records the shape and the pattern, the numeric call checks the pattern and reports whether a
  // full set of min(n_row, n_col) non-zero pivots exists at all — the structural rank over the non-zero entries, where
  // UMFPACK counts the non-zero pivots it found (UMFPACK_WARNING_singular_matrix otherwise) — and holds no factors;
  // the solve returns UMFPACK_ERROR_invalid_system as UMFPACK's does.
  int n_row = 0, n_col = 0;
  bool rectangular = false;
};

// Which factors a Numeric object holds: the one value every reader switches on (spl_umfpack_path is this value plus
// `speculative`).  Written by release_factors (none) and by the three factorisations of umfpack.hip, nowhere else.
//   none          nothing: a rectangular matrix, or between the release of the old factors and the end of a rebuild
//   band_pivoted  LAPACK band storage AB, partial pivoting recorded in ipiv (RCM ordering)
//   band_blocked  blocked band factors without interchanges: AB and blkinv (RCM ordering)
//   tree          multifrontal factors of P A P^T on the nested-dissection tree: mfact (what kind: TreeKind)
//   tree_static   multifrontal factors of B = Dr P A Dc on B's own tree (static pivoting): mfact, spA / spAt, sp_idx / sp_scale
enum class Held { none, band_pivoted, band_blocked, tree, tree_static };
// What the tree factors are (Held::tree; all false for Held::tree_static, whose B is real, unsymmetric and factored
// without interchanges, and for the band kinds).
//   complex_fronts  native complex fronts on ztree, else real fronts on tree
//   ldlt            L D L^T of a symmetric matrix: half the update flops, the transposed system is the system itself
//   block_pivoting  threshold pivoting inside the diagonal blocks of the fronts was on (never with ldlt)
struct TreeKind { bool complex_fronts = false, ldlt = false, block_pivoting = false; };

struct Numeric {
  uint32_t magic = kNumMagic;
  int device = 0;
  int n = 0;
  std::mutex mu;  // the turns of the solves on a speculative object (they may replace the factors)

  // ---- the matrix: set once by the numeric call -------------------------------------------------------------------
  int rectangular = 0;  // 1: of a rectangular matrix (Symbolic::rectangular): no factors, solves return invalid_system
  int singular = 0;     // a zero pivot in the factors held (of the structural / numerical rank when rectangular)
  // 1: diagonally dominant by columns: factors without interchanges are safe.  Otherwise they are a speculation, and the
  // rows of a pivot block of a front are free to change places (TreeKind::block_pivoting; SPL_LU_BLOCK_PIVOT=0: never).
  int dominant = 0;
  // 1: the real embedding E of a complex matrix (umfpack_zi.hip), kept for residuals, refinement and every fallback; its
  // determinant is |det|^2 of the complex matrix.  pair_swap: rows 2r, 2r+1 of E were swapped; pair_unit: complex
  // symmetric matrices, the unit-modulus u_r (re, im) of the congruence D A D.
  int embedding = 0;
  std::vector<char> pair_swap;
  std::vector<double> pair_unit;
  // Native complex fronts (round 3): the tree of the COMPLEX pattern, present when the plain embedding is held and the
  // fronts may be those of the complex matrix itself (half the unknowns, complex fronts in two planes, multifrontal.hip)
  // — a solve with them is a solve with E (packed complex vectors ARE the real vectors of the embedding), at half the
  // flops and bytes.  zsym: the complex matrix is symmetric (A == A^T): L D L^T.
  std::shared_ptr<const mf::Tree> ztree;
  int zsym = 0;
  Matrix *A = nullptr;   // rows of A   (residual b - A x)
  Matrix *At = nullptr;  // rows of A^T (residual b - A^T x)
  std::vector<int> band_perm, band_inv;  // the RCM ordering, kept for the band fallback (empty: ensure_band_ordering)

  // ---- the factors held -----------------------------------------------------------------------------------------------
  Held held = Held::none;
  TreeKind kind;            // of Held::tree
  DBuf<int> perm, inv;      // the ordering of the factors held: RCM for the band kinds, the tree's otherwise
  int kl = 0, ku = 0, ldab = 1;  // band kinds: the bandwidths under RCM and the leading dimension of AB
  DBuf<double> AB;          // band kinds
  DBuf<double> blkinv;      // band_blocked: inv(L11), inv(U11) of every diagonal block
  DBuf<int> ipiv;           // band_pivoted: the row interchanges
  mf::Factors *mfact = nullptr;           // tree kinds
  std::shared_ptr<const mf::Tree> tree;   // tree kinds: the tree of the real fronts (of A's pattern, or of B's)
  DBuf<double> rscale;  // block pivoting: the row scales that rank the candidates (new ordering of the tree in use)
  // tree_static (static_pivot.hpp): spA / spAt: rows of B / of B^T on the device (what mf_factor scatters); sp_idx /
  // sp_scale: the permutations and scalings around a solve with B's factors, composed with B's nested-dissection
  // ordering — [0] before, [1] after A x = b; [2] before, [3] after A^T x = b.
  std::unique_ptr<Matrix> spA, spAt;
  DBuf<int> sp_idx[4];
  DBuf<double> sp_scale[4];
  // 1: the factors held passed the acceptance check a solve runs, made by a determinant call (umfpack_di_get_determinant
  // and the like) on a speculative object: later determinant calls need only the pivot reduction.  Cleared whenever the
  // factors are released.  Solves keep checking as before (speculative is left as it is: ending it would cut their
  // refinement from 10 steps to 2 and their fallbacks off), so a later solve may still replace factors accepted here.
  std::atomic<int> det_checked{0};
  // set when a rebuild failed after the previous factors were released: the object holds no
  // usable factors any more and every later solve returns an error instead of launching kernels
  std::atomic<int> broken{0};

  // ---- the history of the ladder (next_factors, umfpack.hip): every rung is climbed once --------------------------------
  // 1: the matrix is NOT diagonally dominant by columns and the factors held are still a speculation (no interchanges,
  // or static pivoting); solve checks the backward error it computes anyway and, if it is not at rounding level, asks
  // the ladder for the next factors (under `mu`) and solves again.  Cleared when the pivoted band is in place.
  std::atomic<int> speculative{0};
  bool block_pivot_retried = false;  // an L D L^T speculation was factored once more as LU with block pivoting
  bool static_pivot_tried = false;   // static pivoting was attempted, whatever came of it

  // the most recent solve call that finished on this object (spl_umfpack_solve_report; UMFPACK reports the like in
  // Info[UMFPACK_IR_TAKEN .. UMFPACK_OMEGA1]): walks over the factors (first solve + refinement steps, whatever path),
  // refinement steps kept / attempted, largest componentwise backward error among the delivered columns
  std::atomic<int> last_walks{0}, last_ir_taken{0}, last_ir_attempted{0};
  std::atomic<double> last_omega{0.0};
  ~Numeric() {
    delete A;
    delete At;
    if (mfact) mf_free(mfact);
  }
};

// Keeps what spl_umfpack_solve_report describes — the caller's last solve — across solves that are not the caller's
// (the acceptance check of a determinant call, the solves of the condition estimate).
struct KeepSolveReport {
  Numeric *N;
  int walks = N->last_walks, ir_taken = N->last_ir_taken, ir_attempted = N->last_ir_attempted;
  double omega = N->last_omega;
  ~KeepSolveReport() {
    N->last_walks = walks;
    N->last_ir_taken = ir_taken;
    N->last_ir_attempted = ir_attempted;
    N->last_omega = omega;
  }
};

inline Symbolic *as_symbolic(void *p) {
  Symbolic *s = static_cast<Symbolic *>(p);
  return (s && s->magic == kSymMagic) ? s : nullptr;
}
inline Numeric *as_numeric(void *p) {
  Numeric *s = static_cast<Numeric *>(p);
  return (s && s->magic == kNumMagic) ? s : nullptr;
}

// The error boundary of the UMFPACK calls: f's status, or the status of the exception it throws (nothing may cross
// the C ABI).
template <typename F>
int umf_guarded(F &&f) {
  try {
    return f();
  } catch (const DeviceError &e) {
    return e.status == SPL_ERROR_out_of_memory ? UMFPACK_ERROR_out_of_memory : UMFPACK_ERROR_internal_error;
  } catch (const std::bad_alloc &) {
    return UMFPACK_ERROR_out_of_memory;
  } catch (...) {  // e.g. std::system_error from a thread that could not be started
    return UMFPACK_ERROR_internal_error;
  }
}
// the UMFPACK status of an SPL status (sparse_linear_hip.h) returned by the matrix calls behind numeric
inline int umf_status(int spl_status) {
  return spl_status == SPL_ERROR_out_of_memory    ? UMFPACK_ERROR_out_of_memory
         : spl_status == SPL_ERROR_invalid_matrix ? UMFPACK_ERROR_invalid_matrix
                                                  : UMFPACK_ERROR_internal_error;
}

// 64-bit hash of the row indices: the second half of the pattern check in numeric
uint64_t hash_indices(const int *Ai, int64_t nnz);
// Ap[0] == 0, Ap monotone, 0 <= Ai < n_row and ascending in every column: UMFPACK_OK or UMFPACK_ERROR_invalid_matrix
int validate_host_csc(int n_row, int n_col, const int *Ap, const int *Ai);

// The analysis behind umfpack_di_symbolic and, with mult = 2, umfpack_zi_symbolic: (Ap, Ai) is the n x n pattern
// that is ORDERED; the object describes the (n mult) x (n mult) matrix of dense mult x mult blocks whose CSC
// pattern is (Ep, Ei) — what numeric will be handed and checks against.  mult = 1: Ep = Ap, Ei = Ai.
int symbolic_common(int n, const int *Ap, const int *Ai, int mult, const int *Ep, const int *Ei, Symbolic **SymbolicOut);

// Rectangular matrices (Symbolic::rectangular): the analysis records shape and pattern; the "factorisation" checks the
// pattern and counts pivots over the entries nonzero[p] != 0 — with values (re; im null, or packed complex: im = re + 1
// and vstride 2) small matrices get their numerical rank.
int symbolic_rectangular(int n_row, int n_col, const int *Ap, const int *Ai, Symbolic **SymbolicOut);
int numeric_rectangular(Symbolic *S, const int *Ap, const int *Ai, const std::vector<char> &nonzero, Numeric **NumericOut,
                        const double *re = nullptr, const double *im = nullptr, int vstride = 1);

// What the `zi` half tells numeric_factor about the real embedding of a complex matrix; the defaults: a real matrix.
struct EmbeddingOpts {
  bool embedding = false;  // the real embedding of a complex matrix (Numeric::embedding)
  bool native = false;     // the plain embedding, and native complex fronts serve it (Numeric::ztree)
  bool zsym = false;       // ... and the complex matrix is symmetric (Numeric::zsym)
  std::vector<char> pair_swap;    // Numeric::pair_swap
  std::vector<double> pair_unit;  // Numeric::pair_unit
};
// The numeric factorisation of a square matrix whose arguments and pattern the caller has checked; *NumericOut is
// set only when it succeeds (status >= 0).
int numeric_factor(Symbolic *S, const int *Ap, const int *Ai, const double *Ax, EmbeddingOpts opts, Numeric **NumericOut);
// The same with the two device images staged by the caller: stage(N, s, lap) puts the rows of A into N->A and the rows
// of A^T into N->At (on stream s or synchronised; lap names a finished phase for SPL_MF_TIMING) and returns a UMFPACK
// status.  numeric_factor stages them from host arrays; the numeric calls on handles from a handle.  Ap / Ai / Ax: the
// host CSC arrays for static pivoting, or all null — it then reads them back from N->At, as the solves do.
using StageImages = std::function<int(Numeric *N, hipStream_t s, const std::function<void(const char *)> &lap)>;
int numeric_factor_staged(Symbolic *S, EmbeddingOpts opts, const StageImages &stage, const int *Ap, const int *Ai,
                          const double *Ax, Numeric **NumericOut);
// the second image of a stager: N->At from N->A (from_rows) or N->A from N->At, by the device transpose; a UMFPACK status
int stage_transposed_image(Numeric *N, bool from_rows);

// ---- LU from device-resident matrix handles (lu_from_handle.hip; entry points spl_umfpack_{di,zi}_{symbolic,numeric}_dev)
// UMFPACK_OK for a whole-matrix handle with `vw` doubles per value and 32-bit row pointers, else
// UMFPACK_ERROR_invalid_matrix
int handle_status(const Matrix *H, int vw);
// the handle as host CSC arrays (the pattern once for an analysis, the whole matrix on the rectangular route): Ax, when
// not null, receives H->vw doubles per entry
void handle_to_host_csc(const Matrix *H, std::vector<int> &Ap, std::vector<int> &Ai, std::vector<double> *Ax);
void pattern_from_handle(const Matrix *H, DevicePattern &P, hipStream_t s);  // device copy; sets P.ready
// H has exactly the analysed pattern?  P is compared on the device; a host-born analysis (P not ready) first checks H's
// pattern against its own record (column pointers Ap and hash of the row indices) and keeps it as P.
bool handle_has_pattern(const Matrix *H, DevicePattern &P, const std::vector<int> &Ap, uint64_t ai_hash, hipStream_t s);
Matrix *clone_handle(const Matrix *H, hipStream_t s);  // device-to-device copy of the rows image (no SpMV images)
bool complex_handle_symmetric(const Matrix *H, hipStream_t s);  // A == A^T, pattern and bits of the values
// u = sqrt(conj(a) / |a|) of a diagonal entry a = re + i im of a complex symmetric matrix (the congruence D A D of
// umfpack_zi.hip): the root with the non-negative real part, without cancellation; (1, 0) when a is zero or not finite.
// One function for the host route and the handle route: their units have to be the same bits.
inline void congruence_unit(double re, double im, double u[2]) {
  u[0] = 1.0;
  u[1] = 0.0;
  const double mod = std::hypot(re, im);
  if (!std::isfinite(mod) || mod == 0.0) return;
  const double c = re / mod, sn = -im / mod;
  if (c >= 0.0) {
    u[0] = std::sqrt(0.5 * (1.0 + c));
    u[1] = sn / (2.0 * u[0]);
  } else {
    u[1] = std::copysign(std::sqrt(0.5 * (1.0 - c)), sn);
    u[0] = sn / (2.0 * u[1]);
  }
}
// the diagonal of a complex handle: swap flags (|im a_rr| > |re a_rr|; units false) or the unit-modulus u_r of the
// symmetric congruence (units true; computed on the host from the n diagonal entries, see complex_handle_diagonal), on
// the device for the embedding kernel and on the host for the solves
struct ComplexDiagonal {
  DBuf<char> d_swap;
  DBuf<double> d_unit;
  std::vector<char> swap;
  std::vector<double> unit;
  bool any_swap = false;
};
void complex_handle_diagonal(const Matrix *H, bool units, ComplexDiagonal &D, hipStream_t s);
// rows image of the real 2n x 2n embedding of a complex handle (umfpack_zi.hip): plain, swapped pairs (d_swap), or the
// symmetric congruence (d_unit); finalized, synchronised
Matrix *embed_handle(const Matrix *H, const char *d_swap, const double *d_unit, hipStream_t s);

// k systems op(A) X(:,c) = B(:,c) with the factors of N (sys: UMFPACK_A or UMFPACK_At); X and B are n x k
// column-major, in device memory when device_io is set, else on the host.  Info: what umfpack_*_solve reports there.
int solve_columns(Numeric *N, int sys, int k, double *X, const double *B, const int *Ap, const int *Ai,
                  const double *Ax, bool device_io = false, double *Info = nullptr, bool caller_holds_turn = false);

// ---- condition estimate (condest.hip; entry points spl_umfpack_{di,zi}_condest) ----------------------------------------
constexpr int kCondestMaxT = 16;  // columns of the estimator's blocks: 1 .. 16
// k columns op(A) X(:,c) = B(:,c) in device memory, n x k of the value width; returns a UMFPACK status
using DeviceSolve = std::function<int(int sys, int k, double *d_X, const double *d_B)>;
struct CondestResult {
  double norm_inv = 0.0;  // the estimate of ||op(A)^-1||_1: a lower bound the witness reaches
  int iterations = 0, solves = 0, t = 0;
};
// Higham & Tisseur's block estimate of ||op(A)^-1||_1 for an n x n matrix of value width w (1 real, 2 packed complex):
// Y = op(A)^-1 X solves with sys_y, Z = op(A)^-H S with sys_z.  d_witness (n w doubles, may be null): p_inf false: a
// vector x with ||op(A)^-1 x||_1 = est ||x||_1; p_inf true (op(A) = A^T or A^H): x with ||A^-1 x||_inf >= est ||x||_inf.
int condest_inverse_norm(int n, int w, int sys_y, int sys_z, bool p_inf, int t, const DeviceSolve &solve, hipStream_t s,
                         CondestResult &res, double *d_witness);
// the largest sum of |a_ij| over the rows a device matrix holds; width 2: the rows 2g of the real embedding of a complex
// matrix, whose entries pair up into the complex a_gj (umfpack_zi.hip)
double matrix_abs_norm(const Matrix *rows, int width, hipStream_t s);
// The body of spl_umfpack_{di,zi}_condest on a valid square object of the right value kind (umfpack.hip): out[6] as the
// header says, witness (host, N->n doubles: packed for complex objects) when not null.  `solve` runs with the object's
// turn held when it is speculative (solve_columns(..., caller_holds_turn = true)).
int condest_numeric(Numeric *N, int sys, int t, int width, const DeviceSolve &solve, double out[6], double *witness);
// the argument checks of spl_umfpack_{di,zi}_condest (complex_kind: a `zi` object is expected); UMFPACK_OK or the status
int condest_arguments(Numeric *N, bool complex_kind, int sys, int t, const double *out, const void *Ap, const void *Ai,
                      const void *Ax);

}  // namespace spl

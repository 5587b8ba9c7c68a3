/*
 * sparse_linear_hip.h — C ABI of the MI355X (gfx950) backend for the
 * SpMV / SpGEMM / sparse-add / transpose / compress hot path under
 * ttuegel/sparse-linear's Data.Matrix.Sparse.
 *
 * There is no existing FFI for these operations in the reference (they are
 * pure Haskell); the reference's designated seam is
 *   withConstMatrix :: Matrix v a -> (CInt -> CInt -> Ptr CInt -> Ptr CInt -> Ptr a -> IO b) -> IO b
 *       (sparse-linear/src/Data/Matrix/Sparse/Foreign.hs:24-41)   inputs
 *   fromForeign :: Bool -> CInt -> CInt -> Ptr CInt -> Ptr CInt -> Ptr a -> IO (Matrix v a)
 *       (Foreign.hs:43-88)                                           outputs
 * so every matrix crosses this ABI as that 5-tuple
 *   (int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax):
 * CSC, 0-based, int32, Ap[ncols] = nnz, row indices strictly ascending inside
 * a column, borrowed only for the duration of the call.  The LU / solve step
 * keeps its existing link-time ABI: see umfpack_hip.h.
 *
 * Conventions (those of the reference's UMFPACK binding,
 * suitesparse/src/Numeric/LinearAlgebra/Umfpack.hs:60-102):
 *   - every function returns an int status: 0 OK, < 0 fatal (the Haskell
 *     wrapper throws), > 0 warning;
 *   - handles are allocated by the callee and written through a void**; the
 *     free function takes that void**, releases everything and nulls it, and
 *     may be called from any thread (GHC finalizer thread);
 *   - output matrices of unknown size are returned as malloc()'d arrays so
 *     that `fromForeign False` can adopt them (it frees with C free(),
 *     Foreign.hs:54-55); spl_free is free().
 *   - all entry points are thread-safe; a handle may be used from several
 *     threads for read-only operations (spmv) concurrently.
 *
 * No torch / HIP types appear in any signature; `stream` arguments are an
 * opaque hipStream_t passed as void* (NULL = the default stream).
 */
#ifndef SPARSE_LINEAR_HIP_H
#define SPARSE_LINEAR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (UMFPACK's numbering where one exists) ------------------- */
#define SPL_OK 0
#define SPL_WARNING_singular_matrix 1
#define SPL_ERROR_out_of_memory (-1)
#define SPL_ERROR_invalid_handle (-3)
#define SPL_ERROR_argument_missing (-5)
#define SPL_ERROR_n_nonpositive (-6)
#define SPL_ERROR_invalid_matrix (-8)   /* pointers not monotone / index out of range */
#define SPL_ERROR_dimension_mismatch (-20) /* the reference's errorWithStackTrace sites */
#define SPL_ERROR_index_out_of_bounds (-21) /* compress: Sparse.hs:196-212 */
#define SPL_ERROR_index_overflow (-22)  /* result does not fit int32 at the seam */
#define SPL_ERROR_device (-30)          /* HIP runtime failure, no GPU, wrong arch */
#define SPL_ERROR_internal (-911)

/* human-readable name of a status code (static string) */
const char *spl_status_string(int status);
/* number of visible HIP devices (0 if none); never fails */
int spl_device_count(void);
/* last HIP error text seen by this thread ("" if none) */
const char *spl_last_error(void);
void spl_free(void *p);
/* Device blocks of 1 GiB and more (LU factors, fronts, SpGEMM work space) are kept by the library
 * when their owner is freed and reused by the next request they fit, because on this platform a
 * fresh hipMalloc of memory released a moment before waits seconds for the driver's wipe
 * (csrc/device_pool.hip).  They are given back automatically when an allocation of this library
 * fails; this gives them back now (e.g. before another library needs the memory) and returns the
 * number of bytes released.  SPL_CACHE_DEVICE_MEMORY=0 in the environment: never keep any. */
unsigned long long spl_release_cached_memory(void);
/* Seconds this process has spent inside hipMalloc on behalf of the library so far (requests the kept blocks could
 * not serve).  A request that reaches into memory the driver is still wiping — released by this or an earlier
 * process a few seconds before — waits there, and nothing the process has queued on the device runs meanwhile
 * (tools/probe/malloc_overlap_probe.hip): the difference around a call tells how much of it was that wait
 * (benchmarks: the first factorisation of a large matrix against the steady state). */
double spl_device_alloc_seconds(void);

/* ---- one-shot operations on borrowed host CSC 5-tuples ---------------------- */

/* axpy_ (Sparse.hs:433-453):  y <- A x + y.  xlen must equal ncols and ylen
 * nrows, else SPL_ERROR_dimension_mismatch (the reference's two guards). */
int spl_gaxpy(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax,
              int xlen, const double *x, int ylen, double *y);

/* mulV (Sparse.hs:464-471):  y = A x  (y need not be initialised). */
int spl_mulv(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax,
             int xlen, const double *x, double *y);

/* y <- A^T x + y : a pure gather on the CSC arrays. */
int spl_gaxpy_t(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax,
                int xlen, const double *x, int ylen, double *y);

/* mulM (Sparse.hs:473-498): C = A B with B dense brows x bcols, row-major
 * (hmatrix's default order); C is nrows x bcols row-major. */
int spl_mulm(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax,
             int brows, int bcols, const double *B, double *C);
/* mulM on Complex Double (the reference's second SPECIALIZE instance, Sparse.hs:475): Az, Bz and Cz hold packed
 * (re, im) pairs, Bz and Cz row-major as above.  Statuses and guards are spl_mulm's.  Every column of C is
 * bit-identical to one complex axpy_ on that column of B (the kernel of spl_matrix_spmv_many_dev). */
int spl_mulm_z(int nrows, int ncols, const int *Ap, const int *Ai, const double *Az,
               int brows, int bcols, const double *Bz, double *Cz);

/* mm / (*) (Sparse.hs:691-702): C = A B.  Union pattern (cancellation keeps a
 * stored zero), row indices ascending, Cp = exclusive prefix sum.  Outputs are
 * malloc()'d.  SPL_ERROR_index_overflow if nnz(C) >= 2^31 (use the handle API). */
int spl_spgemm(int nrowsA, int ncolsA, const int *Ap, const int *Ai, const double *Ax,
               int nrowsB, int ncolsB, const int *Bp, const int *Bi, const double *Bx,
               int *nrowsC, int *ncolsC, int **Cp, int **Ci, double **Cx);
/* mm on `Matrix U.Vector (Complex Double)` (Sparse.hs:691-702 under the SPECIALIZE of :456-457): values as packed
 * (re, im) pairs; the pattern is that of the real product of the two patterns, every value the sum over ascending k
 * of A[i,k] * B[k,j] in Data.Complex's arithmetic, started from 0 — bit-identical to the Haskell code.  *Cz is
 * malloc()'d with 2 * nnz doubles. */
int spl_spgemm_z(int nrowsA, int ncolsA, const int *Ap, const int *Ai, const double *Az, int nrowsB, int ncolsB,
                 const int *Bp, const int *Bi, const double *Bz, int *nrowsC, int *ncolsC, int **Cp, int **Ci,
                 double **Cz);

/* lin (Sparse.hs:426-431):  C = alpha A + beta B, union pattern. malloc()'d outputs. */
int spl_lin(double alpha, int nrowsA, int ncolsA, const int *Ap, const int *Ai, const double *Ax,
            double beta, int nrowsB, int ncolsB, const int *Bp, const int *Bi, const double *Bx,
            int *nrowsC, int *ncolsC, int **Cp, int **Ci, double **Cx);
/* The same on `Matrix U.Vector (Complex Double)` (the second SPECIALIZE instance, Sparse.hs:456-457; what
 * Feast.hs:216 calls with a complex contour point: `lin (-1) matA _ze matB`): values and the two scalars are
 * (re, im) pairs, products and sums evaluated in Data.Complex's order, so the result is bit-identical to the
 * Haskell code.  *Cz is malloc()'d with 2 * nnz doubles. */
int spl_lin_z(const double alpha[2], int nrowsA, int ncolsA, const int *Ap, const int *Ai, const double *Az,
              const double beta[2], int nrowsB, int ncolsB, const int *Bp, const int *Bi, const double *Bz,
              int *nrowsC, int *ncolsC, int **Cp, int **Ci, double **Cz);

/* transpose (Sparse.hs:301-329): CSC(A) -> CSC(A^T) == CSR(A).  Caller
 * allocates Tp[nrows+1], Ti[nnz], Tx[nnz]. */
int spl_transpose(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax,
                  int *Tp, int *Ti, double *Tx);

/* C = A (x) B, the Kronecker product (`kronecker`, Sparse.hs:597-634): column ja*ncolsB + jb of C
 * holds the rows ia*nrowsB + ib (ascending) with values b*a.  The reference assembles its model
 * problems this way (`kronecker (ident n) T + kronecker T (ident n)`).  Outputs malloc()'d as for
 * spl_spgemm; SPL_ERROR_index_overflow when a dimension or nnz(A)*nnz(B) does not fit int32. */
int spl_kronecker(int nrowsA, int ncolsA, const int *Ap, const int *Ai, const double *Ax, int nrowsB,
                  int ncolsB, const int *Bp, const int *Bi, const double *Bx, int *nrowsC, int *ncolsC,
                  int **Cp, int **Ci, double **Cx);

/* hcat / vcat / fromBlocks / fromBlocksDiag (Sparse.hs:500-595) in one call: nblocks CSC blocks (block b is
 * nrows[b] x ncols[b] with arrays Ap[b], Ai[b], Ax[b]) are placed at (row_off[b], col_off[b]) of an
 * nrowsC x ncolsC result.  Column c of the result is the concatenation, by ascending row offset, of the columns of
 * the blocks that cover it, rows shifted by the block's row offset (vcat's copyWithOffset, Sparse.hs:551-559); the
 * order the blocks are listed in does not matter.  Inside a block's column the entries are moved in the order they
 * have.  hcat: row_off = 0, col_off = running widths; vcat: col_off = 0, row_off = running heights; fromBlocks: both.
 * value_width = 1 (double) or 2 (packed Complex Double: the entries are moved, never combined).  Outputs malloc()'d
 * as for spl_spgemm; SPL_ERROR_dimension_mismatch if a block leaves the result or two blocks overlap,
 * SPL_ERROR_index_overflow if the blocks' entries together do not fit int32. */
int spl_assemble_blocks(int nblocks, const int *nrows, const int *ncols, const int *const *Ap, const int *const *Ai,
                        const double *const *Ax, int value_width, const int *row_off, const int *col_off, int nrowsC,
                        int ncolsC, int **Cp, int **Ci, double **Cx);

/* d[c] = A[c,c], or 0 where no entry is stored, c < min(nrows, ncols) (`takeDiag`, Sparse.hs:636-648) */
int spl_take_diag(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax, double *d);

/* compress / fromTriples (Sparse.hs:184-255): COO -> CSC, duplicates summed,
 * explicit zeros kept.  Ap[ncols+1] caller-allocated; *Ai,*Ax malloc()'d with
 * Ap[ncols] entries.  On SPL_ERROR_index_out_of_bounds *bad is the first
 * offending position (rows checked first, then columns). */
int spl_compress(int nrows, int ncols, int64_t nnz, const int *rows, const int *cols,
                 const double *vals, int *Ap, int **Ai, double **Ax, int64_t *bad);

/* ---- device-resident matrix handles ------------------------------------------ */

/* Upload the CSC 5-tuple once and build the row-major (CSR) image the SpMV
 * kernels read.  The inputs may be freed as soon as the call returns. */
int spl_matrix_create(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax,
                      void **H);
/* The same for Complex Double: Az holds packed (re, im) pairs, 2 * Ap[ncols] doubles (the form the reference
 * passes for its complex instance, Umfpack/Internal.hs:124-132).  On such a handle spl_matrix_mulv / _gaxpy /
 * _spmv_dev take packed complex vectors (2 * ncols and 2 * nrows doubles; xlen, ylen still count entries) and
 * compute  y <- a * x + y  per stored entry in ascending column order with Data.Complex's arithmetic, every
 * real operation separately rounded (csrc/spmv_z.hip: 20 bytes per stored entry instead of the 48 of the real
 * 2n x 2n embedding).  spl_matrix_spmv_many_dev is the fused product of such a handle with k vectors at once.
 * spl_matrix_lin, _transpose, _ctrans, _hermitian, _spgemm, _kronecker, _assemble_blocks, _submatrix, _select, _take_diag_dev, _export_csr,
 * the entry-wise layer (_map, _scale_rows_cols, _filter, _band, _reduce_dev, _norm)
 * and the LU from handles take complex handles as well, and spl_matrix_diag_dev makes one.  Still for real handles only: spl_matrix_export_csc, spl_matrix_export_csr_rows, spl_matrix_spmm_dev and
 * the SpMV images (spl_matrix_build_blocked / _build_panel, the sliced-ELL image; spl_matrix_optimize and
 * spl_matrix_set_variant(H, 0) are accepted and do nothing).  The CSC fields of a complex handle are
 * spl_matrix_export_csr of its spl_matrix_transpose. */
int spl_matrix_create_z(int nrows, int ncols, const int *Ap, const int *Ai, const double *Az, void **H);
/* 1 for a handle made by spl_matrix_create_z, 0 for a real one */
int spl_matrix_is_complex(void *H);
/* Same, but keep only the rows of the part-th of nparts nnz-balanced
 * contiguous row blocks (1-D row partition). */
int spl_matrix_create_rowblock(int nrows, int ncols, const int *Ap, const int *Ai,
                               const double *Ax, int part, int nparts, void **H);
/* Build from CSR arrays directly (== the CSC arrays of A^T). Rows [row0,row0+nrows_local)
 * of a matrix with nrows_global rows.  Column indices need not ascend inside a row: like the CSC entry points the
 * call sorts the rows that do not (indices and values together); rows that already ascend cost one check.
 * Duplicate column indices inside a row are NOT merged (that is spl_compress): they stay separate stored entries,
 * adjacent after the sort and in unspecified relative order.  The SpMV / SpMM kernels add every stored entry;
 * lin, spgemm, transpose, ctrans, hermitian, export_csc and the LU, which rely on strictly ascending indices, are
 * undefined on such a handle. */
int spl_matrix_create_csr(int64_t nrows_global, int64_t ncols, int64_t row0, int64_t nrows_local,
                          const int *rowptr, const int *colidx, const double *val, void **H);
/* Synthetic workloads generated on the device (include/spl_synth.h):
 * kind 0 random(n,K), 1 banded(n), 2 poisson2d(m) [n=m*m], 3 poisson3d(m) [n=m^3].
 * Generates rows [row0,row1) only. */
int spl_matrix_create_synthetic(int kind, int64_t n_or_m, int K, uint64_t seed, int64_t row0,
                                int64_t row1, void **H);
/* R-MAT graph of 2^scale vertices and edge_factor * 2^scale edges with quadrant
 * probabilities (a, b, c, 1-a-b-c); duplicate edges summed (compress semantics). */
int spl_matrix_create_rmat(int scale, int edge_factor, double a, double b, double c, uint64_t seed,
                           void **H);
/* C = A * B on device-resident operands (mm, Sparse.hs:691-702); C gets 64-bit row
 * pointers, so nnz(C) >= 2^31 is fine.  *products (may be NULL) receives the number of
 * intermediate products.  A may be a row block, B must be whole.
 * Two complex handles give a complex C: the pattern of the real product of the two patterns, every value the sum
 * over ascending k of A[i,k] * B[k,j] in Data.Complex's arithmetic, started from 0 — bit for bit spl_spgemm_z.  (The
 * handles hold row-major images, so the column-wise kernel runs with the operands exchanged and forms b * a; with
 * separately rounded operations the packed product is bitwise commutative.)  One real and one complex operand:
 * SPL_ERROR_argument_missing and *HC = NULL (spl_matrix_to_complex first, the rule of spl_matrix_lin). */
int spl_matrix_spgemm(void *HA, void *HB, void **HC, int64_t *products);
void spl_matrix_free(void **H);

/* info[0..7] = nrows_global, ncols, row0, nrows_local, nnz_local, device,
 * rows per panel of the column-blocked image (0 = CSR-stream kernel in use, -64 = sliced-ELL
 * image in use), its cols_log2 */
int spl_matrix_info(void *H, int64_t info[8]);
/* copy the device CSR image back: rowptr[nrows_local+1] (relative to the block,
 * rowptr[0]=0), colidx[nnz_local], val[nnz_local] (2 nnz_local doubles, packed (re, im), for a complex handle) */
int spl_matrix_export_csr(void *H, int64_t *rowptr, int *colidx, double *val);
/* the same for rows [row0, row1) of the block only (a window of a result too large to copy whole):
 * rowptr[row1-row0+1] keeps the block's offsets (rowptr[0] = first entry of row0, not 0); colidx / val
 * receive the rowptr[row1-row0] - rowptr[0] entries of those rows and must hold `capacity` entries
 * (SPL_ERROR_argument_missing if they do not: call once with capacity 0 to learn the count from rowptr) */
int spl_matrix_export_csr_rows(void *H, int64_t row0, int64_t row1, int64_t *rowptr, int64_t capacity, int *colidx,
                               double *val);

/* ---- device-resident forms of lin / transpose / compress: handle in, handle out, nothing crosses PCIe ----
 * spl_matrix_lin: C = alpha A + beta B (Sparse.hs:401-431) for two handles of the same shape, row block and
 *   scalar kind; alpha / beta are (re, im) pairs, the imaginary parts must be 0 for real handles (complex scalars
 *   on real matrices: spl_matrix_to_complex first, as the reference's `cmap (:+ 0)` does, Feast.hs:214).
 * spl_matrix_to_complex: the Complex Double handle (x :+ 0) of a real one.
 * spl_matrix_transpose: handle of A^T (Sparse.hs:301-329), real or complex (the values are moved unchanged); whole
 *   matrices only, a row block is refused with SPL_ERROR_argument_missing.
 * spl_matrix_ctrans: handle of the conjugate transpose, `omap conj . transpose` (Sparse.hs:371-375).  On a real handle
 *   it is spl_matrix_transpose; on a complex one every value arrives as (re, -im), the sign of the imaginary part
 *   flipped as `conjugate` does (+0.0 becomes -0.0), in the same pass that moves the values.  Statuses and refusals
 *   are spl_matrix_transpose's.
 * spl_matrix_hermitian: *result = 1 if `ctrans m == m` under the derived Eq of Sparse.hs:78 (dimensions, pointers,
 *   indices and values, the values with IEEE ==), else 0 (`hermitian`, Sparse.hs:377-379).  Real and complex handles,
 *   whole matrices only.  A matrix that is not square is SPL_OK with *result = 0.  IEEE ==: a NaN anywhere gives 0,
 *   -0.0 equals +0.0 (a real symmetric matrix promoted by spl_matrix_to_complex is Hermitian), a diagonal entry needs
 *   a zero imaginary part, a stored zero whose mirror is not stored gives 0.  The transpose is not built: one kernel
 *   looks every stored entry's mirror up by bisection (csrc/hermitian.hip).  The call synchronises.  Statuses:
 *   SPL_ERROR_invalid_handle; SPL_ERROR_argument_missing (result == NULL, or a row block); SPL_ERROR_index_overflow
 *   (nnz >= 2^31).  Like lin and spgemm it relies on strictly ascending indices: undefined on a handle made by
 *   spl_matrix_create_csr from rows with duplicate indices.
 * spl_matrix_compress_dev: COO triples in DEVICE memory -> handle (compress / fromTriples, Sparse.hs:184-280):
 *   bounds checked rows first, then columns (*bad = first offending position, may be NULL), duplicates summed. */
int spl_matrix_lin(void *HA, const double alpha[2], void *HB, const double beta[2], void **HC);
int spl_matrix_to_complex(void *H, void **HZ);
int spl_matrix_transpose(void *H, void **HT);
int spl_matrix_ctrans(void *H, void **HC);
int spl_matrix_hermitian(void *H, int *result);
int spl_matrix_compress_dev(int nrows, int ncols, int64_t ntriples, const int *d_rows, const int *d_cols,
                            const double *d_vals, void **H, int64_t *bad);
/* ---- the structural constructors on handles: a model problem is assembled where it will be factored --------------
 * Common to the four calls below: operands are whole matrices (a row block: SPL_ERROR_argument_missing, as
 * spl_matrix_transpose answers), all of one value kind and on one device (a real with a complex operand, or two
 * devices: SPL_ERROR_argument_missing and a NULL output; spl_matrix_to_complex first, the rule of spl_matrix_lin).
 * Something that is no matrix handle: SPL_ERROR_invalid_handle.  A NULL output pointer: SPL_ERROR_argument_missing.
 * All argument checks come before the device is touched (without a GPU the calls answer the same up to there, and
 * SPL_ERROR_device after).  The results are ordinary handles — 64-bit row pointers always, int32 ones when nnz fits —
 * and nnz >= 2^31 is fine.  Like lin and spgemm the calls rely on strictly ascending indices in their operands.
 *
 * spl_matrix_kronecker: C = A (x) B (`kronecker`, Sparse.hs:597-634): column ja * ncolsB + jb holds the rows
 *   ia * nrowsB + ib, ia outer, with the values b * a — structure and values bit for bit the reference's; on complex
 *   handles b * a in Data.Complex's order, (br*ar - bi*ai) :+ (br*ai + bi*ar), every real operation rounded once.
 *   Nothing is counted on the device: the row starts and nnz(C) = nnz(A) nnz(B) are known in closed form, one kernel
 *   writes pointers, indices and values.  SPL_ERROR_index_overflow when nrowsA * nrowsB or ncolsA * ncolsB reaches
 *   2^31.  Synchronises (the handle is finished before it is returned, like every result handle).
 * spl_matrix_assemble_blocks: hcat / vcat / fromBlocks / fromBlocksDiag / blockDiag (Sparse.hs:500-595, 661-667) in one
 *   call: block b = H[b] is placed at (row_off[b], col_off[b]) of an nrowsC x ncolsC result.  The blocks are disjoint
 *   rectangles and may be listed in any order: the result does not depend on it.  Blocks without rows or without
 *   columns are legal; nblocks == 0 gives `zeros` (Sparse.hs:673-679) of that shape, real, on the current device.
 *   Values are moved, never combined.  hcat: row_off = 0, col_off = running widths; vcat: col_off = 0, row_off =
 *   running heights; fromBlocks: both; blockDiag: both running.  The number of launches does not depend on nblocks.
 *   Statuses: SPL_ERROR_dimension_mismatch (a block leaves the result, or two blocks overlap: decided on the host from
 *   the rectangles); SPL_ERROR_n_nonpositive (nblocks, nrowsC or ncolsC < 0); SPL_ERROR_index_overflow (nrowsC or
 *   ncolsC >= 2^31); SPL_ERROR_argument_missing (H, row_off or col_off NULL with nblocks > 0).  Synchronises.
 * spl_matrix_take_diag_dev: d_out[c] = A[c,c], or 0 where nothing is stored, c < min(nrows, ncols) (`takeDiag`,
 *   Sparse.hs:640-650).  d_out is DEVICE memory: doubles, or packed (re, im) pairs on a complex handle.  The kernel is
 *   enqueued on `stream`; the call does not synchronise.  d_out == NULL with min(nrows, ncols) > 0:
 *   SPL_ERROR_argument_missing.
 * spl_matrix_diag_dev: `diag` (Sparse.hs:652-659) of n values in DEVICE memory on the current device, value_width 1
 *   (doubles) or 2 (packed pairs: a complex handle).  d_values == NULL: ones, i.e. `ident n` (Sparse.hs:669-671) without
 *   an upload.  n == 0 is the 0 x 0 matrix.  SPL_ERROR_n_nonpositive (n < 0); SPL_ERROR_argument_missing (another
 *   width); SPL_ERROR_index_overflow (n >= 2^31).  Synchronises. */
int spl_matrix_kronecker(void *HA, void *HB, void **HC);
int spl_matrix_assemble_blocks(int nblocks, void *const *H, const int64_t *row_off, const int64_t *col_off,
                               int64_t nrowsC, int64_t ncolsC, void **HC);
int spl_matrix_take_diag_dev(void *H, double *d_out, void *stream);
int spl_matrix_diag_dev(int64_t n, const double *d_values, int value_width, void **H);
/* ---- taking a handle apart: windows, and rows / columns by index (csrc/submatrix.hip) ------------------------------
 * The inverse of spl_matrix_assemble_blocks, under the constructors' common rules: the operand is a whole matrix (a row
 * block: SPL_ERROR_argument_missing), real or complex; the result is an ordinary handle on the operand's device, 64-bit
 * row pointers always, int32 ones when nnz fits; values are moved as bits (NaN payloads, infinities and -0.0 pass
 * unchanged); all argument checks come before the device is touched; the work runs on the default stream and the call
 * synchronises before returning.  Like lin and spgemm both rely on strictly ascending indices in their operand.
 *
 * spl_matrix_submatrix: C[i, j] = A[r0 + i, c0 + j], i < nr, j < nc: C is nr x nc, its indices relative to the window.
 *   This is the operation that the signature and the two guards of the reference's `subMatrix (r0, c0) (nr, nc)`
 *   (Sparse.hs:704-729) document.  The reference's body is untested and does not compute it — `U.slice ix0 nix` passes an
 *   end where a length belongs, the kept row indices are not shifted by r0, and `computePtrs nc _indices` builds column
 *   pointers from row indices — so its bits are NOT reproduced; the documented operation is provided.  Checks, in order:
 *   1. H is no matrix handle: SPL_ERROR_invalid_handle
 *   2. HC == NULL: SPL_ERROR_argument_missing; otherwise *HC = NULL first
 *   3. a negative r0, c0, nr or nc: SPL_ERROR_n_nonpositive
 *   4. r0 + nr > nrows or c0 + nc > ncols: SPL_ERROR_dimension_mismatch (the reference's two errorWithStackTrace sites,
 *      "range exceeds input row size" / "... column size")
 *   5. a row block: SPL_ERROR_argument_missing
 *   nr == 0 or nc == 0 is legal and gives `zeros nr nc`.  Per result row the kept run is found by bisection between
 *   lower_bound(c0) and lower_bound(c0 + nc); nnz(C) is the one 8-byte read-back.  A window of whole rows (c0 == 0,
 *   nc == ncols) searches nothing: a pointer shift and two device-to-device copies.
 * spl_matrix_select: C[i, j] = A[I[i], J[j]]: C is nI x nJ.  d_I and d_J are index arrays in DEVICE memory on the
 *   handle's device, index_width 4 (int32) or 8 (int64) bytes per entry for both; as for spl_matrix_create_csr_dev range
 *   checks are made in the source width BEFORE narrowing (an 8-byte index of 2^32 + 3 is out of bounds, not column 3).
 *   d_I == NULL: all rows in order, and nI must equal nrows; d_J == NULL: the same for the columns.  I may repeat rows
 *   (the rows are copied) and come in any order.  J may come in any order but must not repeat a column.  Every result
 *   row has strictly ascending indices whatever the order of J: when J ascends the rows come out in order and nothing
 *   is sorted, otherwise the rows are sorted, values along with their indices.  Nothing is handed out by atomics: the
 *   result is the same bits from run to run.  A permutation P A Q is I = p, J = q; `toColumns` over a range is
 *   d_I = NULL, J = c0 .. c1; a rank's row block of a matrix assembled on the device is I = row0 .. row1, d_J = NULL.
 *   Checks, in order, 1 - 6 before the device is touched:
 *   1. H is no matrix handle: SPL_ERROR_invalid_handle
 *   2. HC == NULL: SPL_ERROR_argument_missing; otherwise *HC = NULL first
 *   3. a negative nI or nJ: SPL_ERROR_n_nonpositive
 *   4. nI or nJ >= 2^31: SPL_ERROR_index_overflow
 *   5. another index_width, or an array not aligned to its element: SPL_ERROR_argument_missing
 *   6. d_I == NULL with nI != nrows, or d_J == NULL with nJ != ncols: SPL_ERROR_dimension_mismatch
 *   7. a row block: SPL_ERROR_argument_missing
 *   8. an index outside [0, nrows) or [0, ncols): SPL_ERROR_index_out_of_bounds, and *bad (may be NULL) receives the
 *      first offending position; I is checked first, then J, as spl_matrix_compress_dev orders rows and columns
 *   9. a column named twice in J: SPL_ERROR_invalid_matrix
 *   Results that feed the LU keep the project's contract for solves, 1e-10 relative (north_star): a symmetric
 *   permutation select(p, p) of a Hermitian handle is Hermitian, and its factors solve the permuted system. */
int spl_matrix_submatrix(void *H, int64_t r0, int64_t c0, int64_t nr, int64_t nc, void **HC);
int spl_matrix_select(void *H, int64_t nI, const void *d_I, int64_t nJ, const void *d_J, int index_width, void **HC,
                      int64_t *bad);
/* ---- the entry-wise layer on handles: maps, scaling, filters and reductions (csrc/entrywise.hip) --------------------
 * `cmap` / `scale` (Sparse.hs:119-125), the Num instance's negate / abs / signum (Sparse.hs:110-112), conj, the parts
 * and `mag` of Data.Complex.Enhanced, and what a user of handles needs around them: dropping stored zeros, bands and
 * triangles, diag(r) A diag(c), and the abs-sums and norms that produce such scalings.  Common to the six calls:
 * operands are real or complex handles, borrowed and not modified; results that are handles are ordinary handles on the
 * operand's device — 64-bit row pointers always, int32 ones when nnz fits, no SpMV image; every argument check comes
 * before the device is touched (without a GPU the calls answer the same up to there, and SPL_ERROR_device after); the
 * work of the calls that return a handle or a scalar runs on the default stream and they synchronise.  Like lin the
 * calls rely on strictly ascending indices.  A row block is accepted by spl_matrix_map, _scale_rows_cols, _filter,
 * _band and the row-wise reductions, and the result is the same block (same row0 and nrows_global); the column-wise
 * reductions and the norms refuse one with SPL_ERROR_argument_missing.  Every floating-point operation named below is
 * rounded once (no FMA).  Nothing is handed out by atomics and no floating-point atomic add exists: two calls on the
 * same handle give the same bits.
 *
 * magnitude (x :+ y) is GHC's, not hypot:  scaleFloat k (sqrt (sqr (scaleFloat (-k) x) + sqr (scaleFloat (-k) y))),
 *   k = max (exponent x) (exponent y), `exponent` being frexp's exponent and exponent 0 = 0: two ldexp, two products,
 *   one sum, one correctly rounded sqrt, one ldexp.  Pinned bit for bit for finite parts, subnormals and 1e300
 *   included.  With a part that is not finite the result is inf if either part is infinite, else NaN: the reference's
 *   own answer there is an artefact of `decodeFloat` on inf / NaN (a large finite number) and is NOT reproduced.
 *
 * spl_matrix_map: the pattern is copied and one streaming pass runs over the values; stored zeros stay (`cmap` never
 *   prunes).  `scalar` (re, im) is read by SPL_MAP_scale only and may be NULL otherwise.
 *   Real handles, Haskell's results at Double bit for bit: negate flips the sign bit (zeros and NaNs included, payloads
 *   kept); abs clears it; signum is 1 for x > 0, -1 for x < 0, else x itself (+-0 and NaN pass through); conj and real
 *   copy; imag gives the same pattern with +0.0 values; scale gives v * s.
 *   Complex handles, Haskell's at Complex Double: negate negates both parts; conj is (re, -im), the sign bit flipped as
 *   spl_matrix_ctrans does; real and imag return REAL handles; scale is (a :+ b) * (c :+ d) = (ac - bd) :+ (ad + bc)
 *   with v = a :+ b; abs is magnitude z :+ 0 (a complex handle: `omap abs` keeps the type); signum is 0 :+ 0 when z == 0
 *   (IEEE ==), else x / r :+ y / r with r = magnitude z.
 *   Checks, in order:
 *   1. H is no matrix handle: SPL_ERROR_invalid_handle
 *   2. HC == NULL: SPL_ERROR_argument_missing; otherwise *HC = NULL first
 *   3. an unknown op: SPL_ERROR_argument_missing
 *   4. SPL_MAP_scale with scalar == NULL: SPL_ERROR_argument_missing
 *   5. SPL_MAP_scale on a real handle with scalar[1] != 0: SPL_ERROR_argument_missing (the rule of spl_matrix_lin)
 * spl_matrix_scale_rows_cols: C[i,j] = (r[i] * a[i,j]) * c[j], in that order, each product rounded once; on complex
 *   handles r and c are packed (re, im) pairs and the products Data.Complex's, (r * a) then (that * c).  d_r and d_c are
 *   DEVICE memory on the handle's device, nrows_local and ncols entries.  Either may be NULL, meaning ones, and then
 *   that product is not formed at all (bits pass through); both NULL is a copy.  Checks, in order:
 *   1. H is no matrix handle: SPL_ERROR_invalid_handle
 *   2. HC == NULL: SPL_ERROR_argument_missing; otherwise *HC = NULL first
 *   3. a vector not aligned to 8 bytes: SPL_ERROR_argument_missing
 * spl_matrix_filter: a result with fewer entries, the order inside every row kept.  SPL_KEEP_nonzero drops an entry iff
 *   it == 0 (+-0.0 go, NaN stays; a complex entry goes iff both parts == 0); `param` is not read.  SPL_KEEP_abs_above
 *   drops an entry iff |a| <= param[0] (NaN entries stay; complex |a| is the magnitude above, which is 0 for a pair
 *   like 0 :+ 5e-324 — exponent 0 = 0 is the larger exponent and the unscaled square vanishes — so a tolerance of 0
 *   drops a little more than SPL_KEEP_nonzero on complex handles, and the same on real ones).  Two passes: kept entries
 *   counted per row, a scan, a stable compacting write (positions from a ballot); nnz is the one 8-byte read-back.
 *   Checks, in order:
 *   1. H is no matrix handle: SPL_ERROR_invalid_handle
 *   2. HC == NULL: SPL_ERROR_argument_missing; otherwise *HC = NULL first
 *   3. an unknown keep: SPL_ERROR_argument_missing
 *   4. SPL_KEEP_abs_above with param == NULL, or a tolerance that is negative or NaN: SPL_ERROR_argument_missing
 * spl_matrix_band: keeps the entries with lo <= j - i <= hi, i the GLOBAL row (row0 + local row); indices are not
 *   shifted.  INT64_MIN / INT64_MAX open an end; lo > hi gives `zeros` of the operand's shape.  tril(k) is
 *   (INT64_MIN, k), triu(k) is (k, INT64_MAX).  The kept entries are one run per row, found by bisection.  Checks:
 *   1. H is no matrix handle: SPL_ERROR_invalid_handle
 *   2. HC == NULL: SPL_ERROR_argument_missing; otherwise *HC = NULL first
 * spl_matrix_reduce_dev: d_out (DEVICE memory, real doubles for both value kinds) receives per row (axis 1,
 *   nrows_local doubles) or per column (axis 0, ncols doubles) the sum (SPL_REDUCE_abs_sum) or the largest
 *   (SPL_REDUCE_abs_max) of |a| over the stored entries; an empty slice gives +0.0; a NaN in a slice comes out as a
 *   NaN.  The work is enqueued on `stream` and the call does not synchronise, as spl_matrix_take_diag_dev (the column
 *   sums hold temporaries and do synchronise).  A row's sum is formed by its group of lanes in a fixed tree; a column's
 *   sum is the row sum of the order-preserving transpose of the moduli.  For every slice
 *   |got - exact| <= (len + 4) 2^-53 sum|a|.  Checks, in order:
 *   1. H is no matrix handle: SPL_ERROR_invalid_handle
 *   2. an unknown what or axis: SPL_ERROR_argument_missing
 *   3. axis 0 on a row block: SPL_ERROR_argument_missing
 *   4. d_out == NULL (or not aligned to 8 bytes) with a non-empty axis: SPL_ERROR_argument_missing
 *   5. axis 0 with nnz >= 2^31: SPL_ERROR_index_overflow
 * spl_matrix_norm: *result = the 1-norm (largest column abs-sum), the infinity norm (largest row abs-sum), the
 *   Frobenius norm or the max norm (largest |a|) of a whole matrix; no entries: 0.  The Frobenius norm scales by the max
 *   norm first (m sqrt(sum (|a| / m)^2)), so 1e200 or 1e-200 entries give the representable answer; its relative error
 *   is at most (nnz + 4) 2^-53.  Synchronises.  Checks, in order:
 *   1. H is no matrix handle: SPL_ERROR_invalid_handle
 *   2. result == NULL: SPL_ERROR_argument_missing
 *   3. an unknown which: SPL_ERROR_argument_missing
 *   4. a row block: SPL_ERROR_argument_missing
 *   5. SPL_NORM_one with nnz >= 2^31: SPL_ERROR_index_overflow */
#define SPL_MAP_negate 0
#define SPL_MAP_abs 1
#define SPL_MAP_signum 2
#define SPL_MAP_conj 3
#define SPL_MAP_real 4
#define SPL_MAP_imag 5
#define SPL_MAP_scale 6
#define SPL_KEEP_nonzero 0
#define SPL_KEEP_abs_above 1
#define SPL_REDUCE_abs_sum 0
#define SPL_REDUCE_abs_max 1
#define SPL_NORM_one 0
#define SPL_NORM_inf 1
#define SPL_NORM_fro 2
#define SPL_NORM_max 3
int spl_matrix_map(void *H, int op, const double scalar[2], void **HC);
int spl_matrix_scale_rows_cols(void *H, const double *d_r, const double *d_c, void **HC);
int spl_matrix_filter(void *H, int keep, const double param[1], void **HC);
int spl_matrix_band(void *H, int64_t lo, int64_t hi, void **HC);
int spl_matrix_reduce_dev(void *H, int what, int axis, double *d_out, void *stream);
int spl_matrix_norm(void *H, int which, double *result);
/* transpose the block on the device (Sparse.hs:301-329) and copy out its
 * column-major image: colptr[ncols+1], rowidx[nnz_local] (LOCAL row ids, ascending
 * inside a column), val[nnz_local] — i.e. the reference's own CSC Matrix fields */
int spl_matrix_export_csc(void *H, int64_t *colptr, int *rowidx, double *val);

/* ---- compressed arrays and triples that are already in DEVICE memory, in and out: a matrix need not cross PCIe ----
 * The three imports build a handle from arrays on the current device, the two exports write a handle's arrays into
 * device memory the caller allocated (sizes from spl_matrix_info).  A torch.sparse_csr / _csc / _coo tensor on the GPU
 * becomes a handle, and a result handle a tensor, without a host copy (DeviceMatrix.from_torch / to_torch).
 *   index_width  4 (int32) or 8 (int64): the width of the pointer array and of the index array alike
 *   value_width  1 (doubles) or 2 (packed (re, im) pairs: the handle is complex)
 * Imports.  All d_* arguments are device pointers on the current device.  The arrays are borrowed for the call and
 *   copied: they may be freed or overwritten when it returns.  The work runs on the default stream, like that of every
 *   call that makes a handle, and the call synchronises; a caller that filled the arrays on a non-blocking stream
 *   synchronises that stream first (the rule of spl_umfpack_*_solve_many_dev).  The result is a whole-matrix handle like
 *   any other: 64-bit row pointers always, int32 ones when nnz fits, accepted by every operation, the LU from handles
 *   included.  Range checks are made in the source width BEFORE narrowing: with index_width 8 an index of 2^32 + 3 is
 *   out of range, not column 3, and the same holds for pointers.  Values are moved as bits (NaN payloads, infinities,
 *   -0.0 unchanged).
 * spl_matrix_create_csr_dev: the contract of spl_matrix_create_csr for a whole matrix.  rowptr[0] == 0, pointers
 *   monotone, nnz = rowptr[nrows] >= 0, every column in [0, ncols), else SPL_ERROR_invalid_matrix; a last pointer that
 *   promises more entries than the device allocations of d_colidx / d_val hold is refused the same way before they
 *   are read (where the runtime knows the allocation).  Rows whose columns do not ascend are sorted, indices and values
 *   together; a sorted input pays only the check: pointers and indices are each read once and written once, the values
 *   copied once, and nnz is the one 8-byte read-back before the indices.  Duplicate column indices stay separate
 *   entries (the caveat of spl_matrix_create_csr).
 * spl_matrix_create_csc_dev: the reference's own column-major fields, the contract of spl_matrix_create / _create_z
 *   (rows inside a column in any order); the row image is made by the order-preserving device transpose.
 *   nnz >= 2^31: SPL_ERROR_index_overflow, as spl_matrix_export_csc answers.
 * spl_matrix_compress_dev_wide: spl_matrix_compress_dev for 64-bit indices and / or complex values.  Bounds are checked
 *   rows first, then columns; *bad (may be NULL) receives the first offending position, the status is
 *   SPL_ERROR_index_out_of_bounds.  Duplicates are summed in input order, for complex values the real and the imaginary
 *   parts separately in that order (complex addition is componentwise: the reference's compress at Complex Double).
 *   With index_width 4 and value_width 1 the result has the bits of spl_matrix_compress_dev.  ntriples >= 2^31:
 *   SPL_ERROR_index_overflow.
 * Exports.  They write exactly the arrays spl_matrix_export_csr / _export_csc write to the host, with the chosen index
 *   width: pointers[n + 1], indices[nnz], values[nnz * value width].  spl_matrix_export_csr_dev serves row blocks as
 *   spl_matrix_export_csr does (pointers relative to the block).  spl_matrix_export_csc_dev serves complex handles too
 *   (spl_matrix_export_csc still refuses them).  index_width 4 with nnz >= 2^31: SPL_ERROR_index_overflow; the CSC export
 *   answers the same for any width when nnz >= 2^31.  Both run on the default stream and synchronise before returning.
 * Argument checks, all before the device is touched, in this order:
 *   1. H == NULL (imports): SPL_ERROR_argument_missing; otherwise *H = NULL first
 *   2. H is no matrix handle (exports): SPL_ERROR_invalid_handle
 *   3. a negative dimension or count: SPL_ERROR_n_nonpositive
 *   4. nrows or ncols >= 2^31: SPL_ERROR_index_overflow
 *   5. another index_width or value_width, a NULL pointer array, or an array not aligned to its element (4 or 8 bytes):
 *      SPL_ERROR_argument_missing
 *   NULL index or value arrays with nnz > 0 are SPL_ERROR_argument_missing too: for the compressed imports after the
 *   read-back of nnz, for the triples and the exports at once.  Without a GPU a well-formed call answers
 *   SPL_ERROR_device. */
int spl_matrix_create_csr_dev(int64_t nrows, int64_t ncols, int index_width, const void *d_rowptr,
                              const void *d_colidx, const double *d_val, int value_width, void **H);
int spl_matrix_create_csc_dev(int64_t nrows, int64_t ncols, int index_width, const void *d_colptr,
                              const void *d_rowidx, const double *d_val, int value_width, void **H);
int spl_matrix_compress_dev_wide(int64_t nrows, int64_t ncols, int64_t ntriples, int index_width,
                                 const void *d_rows, const void *d_cols, const double *d_vals,
                                 int value_width, void **H, int64_t *bad);
int spl_matrix_export_csr_dev(void *H, int index_width, void *d_rowptr, void *d_colidx, double *d_val);
int spl_matrix_export_csc_dev(void *H, int index_width, void *d_colptr, void *d_rowidx, double *d_val);

/* y = A x  /  y <- A x + y  with HOST vectors (upload, run, download) */
int spl_matrix_mulv(void *H, int xlen, const double *x, double *y);
int spl_matrix_gaxpy(void *H, int xlen, const double *x, int ylen, double *y);

/* Device-resident SpMV: d_x (ncols doubles) and d_y (nrows_local doubles) are
 * DEVICE pointers; the kernel is enqueued on `stream` and the call returns
 * without synchronising.  accumulate != 0: y <- A x + y. */
int spl_matrix_spmv_dev(void *H, const double *d_x, double *d_y, int accumulate, void *stream);
/* Device-resident sparse x dense (mulM): d_B is ncols x k, d_C is nrows_local x k, both
 * row-major DEVICE arrays; A is read once for all k columns.  accumulate != 0: C <- A B + C. */
int spl_matrix_spmm_dev(void *H, const double *d_B, double *d_C, int k, int accumulate, void *stream);
/* Device-resident SpMV on k vectors at once:  Y[:, j] = A X[:, j] (+ Y[:, j] when accumulate != 0),  j = 0 .. k-1.
 * d_X and d_Y are COLUMN-major device arrays — one vector after the other, the layout of the batched solves
 * (spl_umfpack_*_solve_many_dev) — with leading dimensions ldx >= ncols and ldy >= nrows_local counted in entries: a
 * double on a real handle, a packed (re, im) pair on a complex one.  Row-block handles are served (X has ncols rows,
 * Y nrows_local).  X and Y must not overlap; entries of X and Y beyond row ncols / nrows_local of a column are neither
 * read nor written.  The kernel is enqueued on `stream`; the call does not synchronise.  A is read once per 16 vectors.
 * Order: every (row, vector) sum folds  a * x + acc  over the row's stored entries in ascending column order, every
 * real operation separately rounded, the complex product in Data.Complex's order — for rows of ANY length, so vector
 * j's result is the reference's axpy_ on that column bit for bit, and spl_matrix_spmv_dev's in SPL_ORDER_REFERENCE
 * wherever that kernel keeps the order (rows within one chunk of the CSR-stream kernels).  The call always reads the
 * CSR image: spl_matrix_set_spmv_order and the blocked / sliced-ELL / panel images do not change it.  With k = 1 it is
 * no faster than spl_matrix_spmv_dev, and slower on rows longer than a chunk (csrc/spmv_many.hip; measured figures:
 * DESIGN.md).
 * Against spl_matrix_spmm_dev: this call takes column-major vectors and complex handles; that one a row-major real B.
 * Statuses: SPL_ERROR_invalid_handle (H is no matrix handle); SPL_ERROR_n_nonpositive (k < 0); k == 0: SPL_OK, nothing
 * is touched; SPL_ERROR_argument_missing (k > 0 and a needed pointer is NULL or not aligned to an entry, 8 or 16
 * bytes); SPL_ERROR_dimension_mismatch (k > 1 and ldx < ncols or ldy < nrows_local). */
int spl_matrix_spmv_many_dev(void *H, int k, const double *d_X, int64_t ldx, double *d_Y, int64_t ldy,
                             int accumulate, void *stream);
/* ---- sparse triangular solves on handles (csrc/trisolve.hip, csrc/tri_levels.hpp) ----------------------------------
 * T x = b, T^T x = b or T^H x = b for k right-hand sides in device memory, T a triangle of a whole square handle, real
 * or complex: the kernel of Gauss-Seidel / SOR sweeps and of applying an incomplete or externally computed
 * factorisation, between spl_matrix_band (tril / triu) and spl_matrix_spmv_many_dev.
 *   uplo  SPL_TRI_lower: the entries of A with j <= i;  SPL_TRI_upper: those with j >= i.  Entries on the other side of
 *         the diagonal are not read: A need not be triangular (a Gauss-Seidel sweep passes the full matrix).
 *   diag  SPL_DIAG_stored: d_i is the stored a_ii, 0 for a row without one;  SPL_DIAG_unit: d_i = 1, a stored diagonal
 *         is ignored.
 *   op    SPL_OP_n: T x = b;  SPL_OP_t: T^T x = b;  SPL_OP_h: T^H x = b (on a real handle SPL_OP_t).
 * Arithmetic, the contract of spl_matrix_spmv_many_dev: for SPL_OP_n row i computes
 *     acc = b_i;   acc = acc - t_ij * x_j  over the stored off-diagonal entries of row i of T in ASCENDING column order;
 *     x_i = acc / d_i   (unit diagonal: x_i = acc, no division)
 *   with every real operation separately rounded and the division a correctly rounded IEEE division (no stored
 *   reciprocal).  SPL_OP_t / _h run the same loop over the rows of the order-preserving transpose of T (ascending in
 *   the original row index), conjugated first for _h.  Complex handles use Data.Complex's arithmetic:
 *   (a :+ b)(c :+ d) = (a c - b d) :+ (a d + b c), componentwise -, and the scaled quotient
 *     (x :+ y) / (x' :+ y'):  k = -max(e(x'), e(y')), e the frexp exponent and e(0) = 0;  x'' = ldexp(x', k),
 *     y'' = ldexp(y', k);  d = x' x'' + y' y'';  (x x'' + y y'') / d :+ (y x'' - x y'') / d.
 *   The result depends on neither the level schedule nor k nor any launch shape: it is the serial loop bit for bit, for
 *   rows of any length.  A zero or missing diagonal gives what IEEE arithmetic gives (inf, NaN); the solve never refuses.
 * spl_trisolve_analyze: the object is allocated by the callee, written through T, carries its own magic word and is
 *   freed by spl_trisolve_free (idempotent, any thread).  H is borrowed: the object keeps its own device copy of the
 *   triangle, permuted so that the rows of a level are contiguous, and its tables, so H may be freed on return.  The
 *   pattern is downloaded once and the levels, level(i) = 1 + max level(j) over the off-diagonal entries of row i,
 *   computed in one pass on the host; the call runs on the default stream and synchronises.  The launch plan cuts the
 *   levels into segments: a level of at least SPL_TRSV_SMALL_ROWS rows (default 64) is one launch with a group of
 *   lanes per row, a run of smaller levels one launch of a single workgroup that walks at most
 *   SPL_TRSV_SEGMENT_LEVELS levels (default 1024) with a workgroup barrier between them.  Both environment variables
 *   are read once per analysis and clamped (1 ... 2^30, 1 ... 65536).  No kernel waits for another workgroup.
 *   Returns SPL_OK, or SPL_WARNING_singular_matrix (1, the object exists) when diag is SPL_DIAG_stored and some d_i is
 *   missing or exactly zero (complex: both parts).  Errors, checked in this order before the device is touched:
 *   SPL_ERROR_invalid_handle (H is NULL or no matrix handle); SPL_ERROR_argument_missing (T is NULL or a code is
 *   unknown; otherwise *T = NULL first); SPL_ERROR_dimension_mismatch (not square); SPL_ERROR_invalid_matrix (a
 *   row-block handle, or one without 32-bit row pointers, nnz >= 2^31); then SPL_ERROR_device without a GPU.
 * spl_trisolve_solve_dev: d_B and d_X are COLUMN-major device arrays with leading dimensions ldb, ldx counted in
 *   entries (a double, or a packed pair), the layout of spl_matrix_spmv_many_dev.  d_X == d_B with ldx == ldb (in
 *   place) is allowed; any other overlap is undefined.  Entries beyond row n of a column are neither read nor written.
 *   The kernels are enqueued on `stream` and the call does not synchronise — except the FIRST call with SPL_OP_t or
 *   SPL_OP_h, which builds the transposed image and its schedule on the default stream and synchronises; later calls
 *   do not.  The right-hand sides go through in groups of 8; every column has the bits of a single-column solve.
 *   Concurrent solves on one object from several host threads are safe (no scratch; the lazy build runs under a lock).
 *   Statuses: SPL_ERROR_invalid_handle (T is no such object); SPL_ERROR_n_nonpositive (k < 0); k == 0 or n == 0:
 *   SPL_OK, nothing is touched; SPL_ERROR_argument_missing (op unknown, a pointer NULL or not aligned to an entry, 8
 *   or 16 bytes); SPL_ERROR_dimension_mismatch (k > 1 and ldb < n or ldx < n).
 * spl_trisolve_solve: the same with HOST arrays, n x k column-major without padding, packed complex; B == X is allowed.
 * spl_trisolve_info: [0] n, [1] stored entries of the triangle (stored diagonals included, also with a unit diagonal),
 *   [2] levels, [3] kernel launches one SPL_OP_n solve of up to 8 columns makes, [4] rows i with d_i missing or zero (0
 *   with a unit diagonal), [5] longest row of the triangle (counted as [1]), [6] bytes of device memory held, [7] flags:
 *   bit 0 complex, bit 1 upper, bit 2 unit diagonal, bit 3 a transposed image is built. */
#define SPL_TRI_lower 0
#define SPL_TRI_upper 1
#define SPL_DIAG_stored 0
#define SPL_DIAG_unit 1
#define SPL_OP_n 0
#define SPL_OP_t 1
#define SPL_OP_h 2
int spl_trisolve_analyze(void *H, int uplo, int diag, void **T);
int spl_trisolve_solve_dev(void *T, int op, int k, const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                           void *stream);
int spl_trisolve_solve(void *T, int op, int k, const double *B, double *X);
int spl_trisolve_info(void *T, int64_t info[8]);
void spl_trisolve_free(void **T);

/* ---- ILU(0) on handles (csrc/ilu0.hip, csrc/tri_levels.hpp) ----------------------------------------------------------
 * The incomplete LU factorisation without fill of a whole square handle, real or complex: the producer of what the
 * triangular solves above apply.  L (unit lower, its ones not stored) and U live in ONE ordinary matrix handle F with
 * A's own pattern, so F goes to spl_trisolve_analyze as it is: (F, SPL_TRI_lower, SPL_DIAG_unit) is L and
 * (F, SPL_TRI_upper, SPL_DIAG_stored) is U, and M^-1 b = U^-1 (L^-1 b) is two spl_trisolve_solve_dev calls.
 * Arithmetic: the serial IKJ loop on a copy of A's values, rows in CSR order with strictly ascending columns,
 *     for i = 0 ... n-1:
 *       for each stored (i,k) with k < i, ascending k:
 *         a_ik = a_ik / u_kk              u_kk: the final stored diagonal of row k, 0 when row k stores none
 *         for each stored (i,j) with j > k, ascending j:
 *           if (k,j) is stored in row k:   a_ij = a_ij - a_ik * a_kj
 *   with every real operation separately rounded and the division a correctly rounded IEEE division (no stored
 *   reciprocal); complex handles use Data.Complex's product and scaled quotient, exactly those of the triangular
 *   solves above.  Every entry receives its updates in ascending k, each one product and one difference, so the result
 *   depends on neither the level schedule nor the lanes a row gets nor any launch shape: it is the serial loop bit for
 *   bit, for rows of any length.  A zero or missing pivot gives what IEEE arithmetic gives (inf, NaN); the
 *   factorisation never refuses on values.
 * spl_ilu0_analyze: the plan is allocated by the callee, written through P, carries its own magic word and is freed by
 *   spl_ilu0_free.  H is borrowed: the plan keeps its own device copy of the pattern (row pointers, columns), the
 *   positions of the diagonals and the level tables, and no values, so H may be freed on return and ONE plan factors
 *   real and complex handles alike.  The pattern is downloaded once; row i waits for the rows k < i of its lower
 *   pattern, which is the dependency structure of the lower triangular solve, and the levels and the launch plan are
 *   those of spl_trisolve_analyze (SPL_TRSV_SMALL_ROWS, SPL_TRSV_SEGMENT_LEVELS, read once per analysis; the lanes per
 *   row follow the mean length of the whole rows).  The call runs on the default stream and synchronises.  No kernel
 *   waits for another workgroup.  Returns SPL_OK.  Errors, checked in this order before the device is touched:
 *   SPL_ERROR_invalid_handle (H is NULL or no matrix handle); SPL_ERROR_argument_missing (P is NULL; otherwise
 *   *P = NULL first); SPL_ERROR_dimension_mismatch (not square); SPL_ERROR_invalid_matrix (a row-block handle, or one
 *   without 32-bit row pointers, nnz >= 2^31); then SPL_ERROR_device without a GPU.
 * spl_ilu0_factor: F receives a NEW ordinary matrix handle (freed by spl_matrix_free) with the pattern of H and the
 *   L\U values, real when H is real and complex when H is complex.  H may be ANY whole handle with the analysed
 *   pattern: new values on an old pattern are a refactorisation without an analysis.  The pattern is compared on the
 *   device (n, nnz, then every row pointer and column); a difference gives SPL_ERROR_invalid_matrix and no F.  The call
 *   runs on the default stream and synchronises.  Returns SPL_OK, or SPL_WARNING_singular_matrix (1, F exists) when
 *   some final u_kk is missing or exactly zero (complex: both parts).  Concurrent factorisations on one plan from
 *   several host threads are safe (the plan holds no scratch).  Errors: SPL_ERROR_invalid_handle (P is no plan or H no
 *   matrix handle); SPL_ERROR_argument_missing (F is NULL; otherwise *F = NULL first); SPL_ERROR_invalid_matrix (H is a
 *   row block, has no 32-bit row pointers, lies on another device, or has another pattern).
 * spl_ilu0_info: [0] n, [1] nnz, [2] levels, [3] kernel launches one factorisation makes, [4] rows without a stored
 *   diagonal, [5] longest row, [6] bytes of device memory held, [7] factorisations done so far.
 * spl_ilu0_free: idempotent, any thread; NULL and a pointer to NULL are accepted; a pointer to what is no plan is
 *   nulled and nothing is released.
 * spl_matrix_ilu0: analyze + factor + free in one call, with the statuses of the two. */
int spl_ilu0_analyze(void *H, void **P);
int spl_ilu0_factor(void *P, void *H, void **F);
int spl_ilu0_info(void *P, int64_t info[8]);
void spl_ilu0_free(void **P);
int spl_matrix_ilu0(void *H, void **F);

/* ---- the fixed-order inner product, preconditioned CG and BiCGSTAB on handles (csrc/krylov.hip) -----------------------
 * A x = b on the device without a factorisation of A: the operator is spl_matrix_spmv_dev on a whole square handle, real
 * or complex, the preconditioner is made of the objects above, and every scalar of the iteration stays in device memory.
 * The contract is the one of the other handle operations: the result is a serial restatement's bit for bit, whatever
 * the launch shapes are.
 *
 * fold(v, len): v is cut into chunks of 4096 consecutive entries, the last one may be short.  In a chunk, lane t of 256
 *   starts from +0.0 and adds the entries t, t + 256, t + 512 ... in ascending order; the 256 lane sums are then folded
 *   as s[t] = s[t] + s[t + h], t < h, for h = 128, 64 ... 1, and s[0] is the chunk's partial.  The partials are folded
 *   by the same fold until one value is left (two levels up to 4096^2 entries, three beyond); fold of nothing is +0.0.
 * <a,b> = fold of the entry-wise products: a_i * b_i on real vectors, conj(a_i) * b_i with Data.Complex's product
 *   ((a :+ b) * (c :+ d) = (a c - b d) :+ (a d + b c), applied to (a_re, -a_im) and b) on packed complex ones, the real
 *   and the imaginary parts folded apart; every real operation separately rounded.  |r|^2 is the real part of <r,r>.
 *   The order is a function of len alone: no floating-point atomic, no kernel that waits for another workgroup, and
 *   the grid (SPL_KRYLOV_GRID, workgroups of a chunk kernel at most, default 2048) does not show in the bits.
 * spl_vector_dot_dev: d_out[0] (and d_out[1], value_width 2) = <a,b> of n entries of value_width doubles each, all in
 *   DEVICE memory.  Enqueued on `stream`, no synchronisation.  Every CALL takes a block of its own from the device pool
 *   for the partials (one whose previous user has finished on the device, told by an event recorded behind that user's
 *   last kernel, or a new one), so calls from several host threads, on one stream or on several, never share partials;
 *   a handful of finished blocks is kept for reuse, whatever the number of streams and calls.  n < 0: SPL_ERROR_n_nonpositive; n == 0 writes +0.0; a value_width outside {1, 2}, a NULL pointer
 *   (d_a, d_b with n > 0; d_out always) or one not aligned to an entry (8 or 16 bytes): SPL_ERROR_argument_missing.
 *
 * spl_krylov_create: the object is allocated by the callee, written through K, carries its own magic word and is freed
 *   by spl_krylov_free (idempotent, any thread; NULL, a pointer to NULL and a pointer to what is no such object are
 *   accepted).  A is BORROWED and must outlive K; the operator is spl_matrix_spmv_dev on A as the caller configured it
 *   (images, variant, order mode).  In SPL_ORDER_FREE the SpMV's sums are not in the reference's order and the bit
 *   contract of this section is VOID; everything else holds.  (In SPL_ORDER_REFERENCE the SpMV's own caveats apply: a row
 *   of more than 512 entries is summed by a wavefront tree.)  The object owns its work vectors (4 for CG, 8 for
 *   BiCGSTAB), the partials of the fold and a status block in device memory: iteration counter, done, reason, rho,
 *   alpha, beta, omega, |r|^2, |b|^2, the threshold.  Solves on one object are serialised under its lock.
 *   Errors, checked in this order before the device is touched: SPL_ERROR_invalid_handle (A is NULL or no matrix
 *   handle); SPL_ERROR_argument_missing (K is NULL; otherwise *K = NULL first; then an unknown method);
 *   SPL_ERROR_dimension_mismatch (not square); SPL_ERROR_invalid_matrix (a row-block handle); then SPL_ERROR_device
 *   without a GPU.
 * spl_krylov_set_preconditioner: z = M^-1 r = T2^-1 (d_mid (.) (T1^-1 r)), every part may be NULL (the identity).  T1
 *   and T2 are spl_trisolve objects, applied with SPL_OP_n and k = 1; d_mid is a DEVICE vector of n entries (packed
 *   pairs on a complex object), multiplied entry by entry, d_mid_i * v_i (Data.Complex's product).  All are borrowed.
 *   No preconditioner: all NULL.  Jacobi: d_mid = 1 / diag(A).  ILU(0): T1 = (F, lower, unit), T2 = (F, upper, stored).
 *   Symmetric Gauss-Seidel: T1 = (A, lower, stored), d_mid = diag(A), T2 = (A, upper, stored).  Errors:
 *   SPL_ERROR_invalid_handle (K, or a part that is not NULL, is no such object); SPL_ERROR_argument_missing (d_mid not
 *   aligned to an entry); SPL_ERROR_dimension_mismatch (a triangular object of another size, value kind or device).
 * The scalars: q = a / b is the IEEE division, on complex objects Data.Complex's scaled quotient (that of the
 *   triangular solves); every vector update is one product and one sum or difference per entry, each rounded once:
 *   x_i = x_i + alpha * p_i.  A scalar is zero when all its parts are, non-finite when one part is.
 *   threshold = max(rtol * sqrt(|b|^2), atol);  met(v): sqrt(v) <= threshold.
 * SPL_KRYLOV_cg, standard preconditioned CG:
 *     r = b - A x   (use_x0 == 0: r = b and x = 0, no SpMV);  it = 0;  history[0] = sqrt(|r|^2)
 *     |r|^2 or |b|^2 not finite: reason 3;  met(|r|^2): reason 0;  max_iter == 0: reason 1
 *     z = M^-1 r;  rho = <r,z>  (zero or non-finite: reason 2);  p = z
 *     repeat:  q = A p;  d = <p,q>  (zero or non-finite: reason 2);  alpha = rho / d
 *              x = x + alpha p;  r = r - alpha q;  it = it + 1;  history[it] = sqrt(|r|^2)
 *              |r|^2 not finite: reason 3;  met(|r|^2): reason 0;  it == max_iter: reason 1
 *              z = M^-1 r;  rho' = <r,z>  (zero or non-finite: reason 2);  beta = rho' / rho;  rho = rho'
 *              p = z + beta p
 *   Without a preconditioner z is r, and <r,z> is the <r,r> the residual step has just folded, bit for bit (both
 *   parts, when complex): it is not computed again.
 * SPL_KRYLOV_bicgstab, van der Vorst's method, preconditioned from the right:
 *     r = b - A x as above, rhat = r, the same checks of iteration 0
 *     repeat:  rho' = <rhat,r>  (zero or non-finite: reason 2)
 *              first pass: p = r;  later: beta = (rho' / rho) * (alpha / omega);  p = r + beta (p - omega v)
 *              rho = rho';  y = M^-1 p;  v = A y;  d = <rhat,v>  (zero or non-finite: reason 2);  alpha = rho / d
 *              s = r - alpha v;  x = x + alpha y
 *              |s|^2 not finite: reason 3;  met(|s|^2): it = it + 1, history[it] = sqrt(|s|^2), reason 0
 *              z = M^-1 s;  t = A z;  omega = <t,s> / <t,t>  (<t,t> or omega zero or non-finite: reason 2)
 *              x = x + omega z;  r = s - omega t;  it = it + 1;  history[it] = sqrt(|r|^2)
 *              |r|^2 not finite: reason 3;  met(|r|^2): reason 0;  it == max_iter: reason 1
 *   The first reason met ends the solve: nothing after it is computed, x is the iterate of that moment (after a
 *   breakdown behind BiCGSTAB's half step x holds the half step, and it counts the completed iterations).  A breakdown
 *   never hangs and never refuses.
 * spl_krylov_solve_dev: d_b and d_x are DEVICE vectors of n entries, not the same array; use_x0 != 0 takes d_x as the
 *   start, otherwise d_x is only written.  The kernels are enqueued on `stream`.  Convergence is decided on the device:
 *   the kernel that completes |r|^2 sets `done`, and every vector kernel of the solver returns without touching a
 *   vector once it is set.  The host copies the status block into pinned memory and synchronises `stream` every
 *   check_every iterations (0: the default, 16) and stops launching once `done` is set, so x, the iteration count and
 *   the history do NOT depend on check_every; only the launches issued for nothing do.  The call returns after a last
 *   synchronisation.  result = {iterations, reason (0 converged, 1 max_iter, 2 breakdown, 3 non-finite), SpMVs issued,
 *   preconditioner applications issued}.  history may be NULL; otherwise it is a HOST array of max_iter + 1 doubles
 *   that receives sqrt(|r_it|^2) of the recurrence for it = 0 ... iterations.  On the device the history takes room
 *   for the iterations that were ISSUED (grown at the looks at the status block), not for max_iter: a large max_iter
 *   as "no limit" costs nothing there; the host array is the caller's.  Returns SPL_OK whenever it ran: the
 *   outcome is in result.  b = 0 (and no start) gives x = 0 after 0 iterations, reason 0.  n == 0: SPL_OK, result all
 *   0, history[0] = 0.  Errors, in this order: SPL_ERROR_invalid_handle (K); SPL_ERROR_argument_missing (result NULL);
 *   SPL_ERROR_n_nonpositive (max_iter < 0); SPL_ERROR_argument_missing (rtol or atol negative or NaN, check_every < 0);
 *   SPL_ERROR_index_overflow (a history of 2^31 entries or more); SPL_ERROR_argument_missing (d_b or d_x NULL, the
 *   same, or not aligned to an entry).
 * spl_krylov_solve: the same with HOST vectors (packed complex), on the default stream with the default check_every;
 *   x is read only with use_x0 != 0.
 * spl_krylov_info: [0] n, [1] method, [2] flags (1 complex, 2 T1 set, 4 d_mid set, 8 T2 set), [3] bytes of device memory
 *   held, [4] solves so far, [5] iterations of the last solve, [6] kernel launches per iteration of the last solve (the
 *   SpMV counted as one), [7] reserved, 0. */
#define SPL_KRYLOV_cg 0
#define SPL_KRYLOV_bicgstab 1
int spl_vector_dot_dev(int64_t n, int value_width, const double *d_a, const double *d_b, double *d_out, void *stream);
int spl_krylov_create(void *A, int method, void **K);
int spl_krylov_set_preconditioner(void *K, void *T1, const double *d_mid, void *T2);
int spl_krylov_solve_dev(void *K, const double *d_b, double *d_x, int use_x0, double rtol, double atol, int64_t max_iter,
                         int check_every, int64_t result[4], double *history, void *stream);
int spl_krylov_solve(void *K, const double *b, double *x, int use_x0, double rtol, double atol, int64_t max_iter,
                     int64_t result[4], double *history);
int spl_krylov_info(void *K, int64_t info[8]);
void spl_krylov_free(void **K);

/* ---- multicolour ordering on handles (csrc/coloring.hip) --------------------------------------------------------------
 * The levels of a triangular solve and of ILU(0) are a property of the ordering.  Colour the adjacency graph so that no
 * two neighbours share a colour and number the unknowns colour by colour: a row of the lower triangle of P A P^T then
 * depends on rows of earlier colours only, and spl_trisolve_analyze / spl_ilu0_analyze find at most as many levels as
 * there are colours.  The price is convergence: a multicolour ILU(0) or Gauss-Seidel is a weaker preconditioner.
 *
 * Graph: the vertices are 0 ... n-1; {i, j}, i != j, is an edge when a_ij or a_ji is stored, stored zeros included.
 *   Values are never read: a real and a complex handle of one pattern give the same result.
 * Priority: h(v) = the splitmix64 finaliser of v + 0x9E3779B97F4A7C15 (seed + 1), all mod 2^64:
 *     z = v + 0x9E3779B97F4A7C15 (seed + 1);  z = (z ^ z >> 30) 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) 0x94D049BB133111EB;
 *     h = z ^ z >> 31
 *   u PRECEDES v when h(u) > h(v), or when they are equal and u < v: a strict total order.
 * colour(v) = the smallest c >= 0 that no neighbour preceding v has;
 * round(v)  = 1 + the largest round(u) over the neighbours u that precede v, 1 when there are none.
 *   The colours are those of the serial first-fit colouring taken in priority order, which is the fixed point of
 *   Jones-Plassmann rounds: functions of the pattern and the seed alone.  d_colors holds exactly those integers, whatever
 *   the grid (SPL_COLOR_GRID, workgroups of a launch at most, default 2048), the order of the worklist and the host's
 *   looks at it are.
 * spl_matrix_color: order must be SPL_COLOR_hash.  d_colors: n int32 in DEVICE memory.  d_perm (may be NULL): n int32 in
 *   device memory; perm[k] is the old index of new row k, the vertices sorted by colour and then by ascending index (the
 *   stable order), the form spl_matrix_select takes as I and J: P A P^T = select(A, perm, perm).  *offsets (offsets may
 *   be NULL): a HOST array of info[1] + 1 int64 with the class boundaries in perm, allocated by the callee and released
 *   with spl_free.  One launch is one round: every vertex of the worklist whose preceding neighbours all carried a
 *   colour when the launch began takes its colour.  No kernel waits for another workgroup.  The host reads the number
 *   of vertices left every SPL_COLOR_CHECK_EVERY rounds (read once per call, 1 ... 4096, default 8); a round on an empty
 *   worklist does nothing.  The call runs on the default stream and synchronises.
 *   info: [0] n, [1] colours, [2] rounds = the largest round(v), [3] largest class, [4] smallest class, [5] largest
 *   degree of the graph, [6] kernel launches of csrc/coloring.hip issued (those inside the scan and the sort are not
 *   counted), [7] 0.  n == 0: SPL_OK, 0 colours, offsets = {0}.  No off-diagonal entry: one colour, the identity.
 *   Errors, checked in this order before the device is touched: SPL_ERROR_invalid_handle (H is NULL or no matrix
 *   handle); SPL_ERROR_argument_missing (d_colors or info is NULL; *offsets = NULL first when offsets is given);
 *   SPL_ERROR_argument_missing (an unknown order, or d_colors / d_perm not aligned to 4 bytes);
 *   SPL_ERROR_dimension_mismatch (not square); SPL_ERROR_invalid_matrix (a row-block handle, or one without 32-bit row
 *   pointers, nnz >= 2^31); then SPL_ERROR_device without a GPU.
 * spl_vector_permute_dev: out[k] = in[perm[k]] (inverse == 0) or out[perm[k]] = in[k] (inverse != 0) for n entries of
 *   value_width doubles (1, or 2: packed complex), all in DEVICE memory, moved as bits; d_in and d_out are different
 *   arrays.  perm is trusted: it is the array spl_matrix_color wrote.  Enqueued on `stream`, no synchronisation.
 *   n < 0: SPL_ERROR_n_nonpositive; n == 0 does nothing; a value_width outside {1, 2}, with n > 0 a NULL pointer or
 *   d_in == d_out, a pointer not aligned to its entries (4, and 8 or 16 bytes): SPL_ERROR_argument_missing. */
#define SPL_COLOR_hash 0
int spl_matrix_color(void *H, int order, uint64_t seed, int *d_colors, int *d_perm, int64_t **offsets, int64_t info[8]);
int spl_vector_permute_dev(int64_t n, int value_width, const int *d_perm, int inverse, const double *d_in, double *d_out,
                           void *stream);

/* ---- aggregation AMG on handles (csrc/amg.hip) --------------------------------------------------------------------------
 * A multigrid cycle is a short sequence of SpMVs and vector updates per level, and it cuts the iteration count of CG and
 * BiCGSTAB by an order of magnitude where ILU(0) walks hundreds of dependent levels.  The hierarchy is smoothed (or
 * plain) aggregation on the constant, built handle to handle from the public operations above, so every level's bits
 * are defined by theirs; the cycle is a fixed linear operator with the Krylov section's bit contract.
 *
 * spl_matrix_aggregate.  Graph and priority are EXACTLY those of spl_matrix_color: {i, j}, i != j, is an edge when a_ij
 *   or a_ji is stored, stored zeros included; values are never read; h(v) is the same finaliser with the same seed
 *   formula; u precedes v when h(u) > h(v), or they are equal and u < v.
 *   Roots: the greedy maximal independent set of distance 2 in priority order.  Walk the vertices in priority order; an
 *   undecided vertex becomes a root, and every undecided vertex within graph distance <= 2 of it is out (paths run
 *   through any vertex, decided or not).  The device finds them in rounds: every undecided vertex that precedes all
 *   other vertices within distance <= 2 that were undecided WHEN THE ROUND BEGAN becomes a root, then every undecided
 *   vertex within distance <= 2 of a new root is out.  Roots and round count are functions of the pattern and the seed
 *   alone.  A round is four launches (two propagations of the first undecided vertex over closed neighbourhoods, two
 *   marking passes), each reading what the one before it finished; no kernel waits for another workgroup, there is no
 *   floating-point operation, and the integer atomics only count.  Neither the grid (SPL_AMG_GRID, workgroups of a
 *   launch at most, default 2048) nor the host's check interval (SPL_AMG_CHECK_EVERY rounds between two looks at the
 *   number of undecided vertices, 1 ... 4096, default 8; a round that finds nobody undecided does nothing) shows in any
 *   output.
 *   Aggregates: aggregate k is rooted at the k-th root in ascending vertex index.  Phase 1: every neighbour of a root
 *   joins that root (unique: two roots are never within distance 2).  Phase 2: every remaining vertex takes the
 *   aggregate of that neighbour, among its neighbours assigned in phase 1, which precedes the others (one exists, by
 *   maximality).  A vertex without edges is its own aggregate.
 *   d_agg: n int32 in DEVICE memory.  d_roots (may be NULL): n int32 in device memory, of which the first info[1] are
 *   written.  info: [0] n, [1] aggregates, [2] rounds, [3] largest aggregate, [4] smallest aggregate, [5] largest
 *   degree, [6] kernel launches of csrc/amg.hip issued, [7] vertices assigned in phase 2.  n == 0: SPL_OK, 0 aggregates.
 *   The handle may be real or complex.  The call runs on the default stream and synchronises.  Errors, in this order
 *   before the device is touched: SPL_ERROR_invalid_handle; SPL_ERROR_argument_missing (d_agg or info NULL);
 *   SPL_ERROR_argument_missing (d_agg / d_roots not aligned to 4 bytes); SPL_ERROR_dimension_mismatch (not square);
 *   SPL_ERROR_invalid_matrix (a row-block handle, or one without 32-bit row pointers); then SPL_ERROR_device.
 *
 * spl_amg_create.  opt (may be NULL: all 0): [0] seed; [1] sweeps nu, 0 -> 1, allowed 1 ... 4; [2] coarse_size, 0 -> 256;
 *   [3] max_levels, 0 -> 16, allowed 1 ... 64; [4] coarse_sweeps, 0 -> 4, allowed 1 ... 64; [5] flags, bit 0: plain
 *   (unsmoothed) prolongator; [6], [7] must be 0.  A_0 = A is BORROWED and must outlive M.  Level l with matrix A_l of
 *   n_l rows is the composition of the public handle operations, in this order:
 *     1. d = take_diag(A_l);  dinv_i = 1 / d_i  (IEEE division; Data.Complex's quotient of (1 :+ 0) on complex handles)
 *     2. nrm = norm_inf(scale_rows_cols(A_l, r = dinv))
 *     3. omega = 4.0 / (3.0 * nrm), two rounded operations
 *     4. w_i = omega * dinv_i  ((omega :+ 0) times dinv_i by Data.Complex's product on complex handles)
 *     5. the level is the coarsest when n_l <= coarse_size, or l + 1 == max_levels, or aggregation gives n_{l+1} == n_l
 *     6. agg = spl_matrix_aggregate(A_l, seed);  T = the n_l x n_{l+1} handle with one entry 1.0 per row at column
 *        agg[i], made by spl_matrix_create_csr_dev
 *     7. P = lin(1, T, -1, spgemm(scale_rows_cols(A_l, r = w), T));  plain: P = T
 *     8. R = ctrans(P)  (transpose on real handles)
 *     9. A_{l+1} = spgemm(R, spgemm(A_l, P)), in that association
 *   A zero or missing diagonal gives inf / NaN in w and sets bit 0 of spl_amg_info's [7]: a warning, never a refusal
 *   (ILU(0)'s policy); the solve that uses such a cycle ends with a non-finite outcome.  M owns every level's handles
 *   but A_0, the weights and the work vectors.  Setup runs on the default stream and synchronises.  Errors, before
 *   the device is touched: SPL_ERROR_invalid_handle; SPL_ERROR_argument_missing (M NULL; otherwise *M = NULL first);
 *   SPL_ERROR_argument_missing (an option out of range or a reserved one nonzero); SPL_ERROR_dimension_mismatch (not
 *   square); SPL_ERROR_invalid_matrix (a row-block handle, or one without 32-bit row pointers); then SPL_ERROR_device.
 * spl_amg_level lends level `level`: *HA, *HP, *HR (P and R NULL on the coarsest level), *d_w (the device vector of n_l
 *   entries) and dims = {n_l, n_{l+1} or 0}; every output may be NULL.  The handles are M's: they are not freed by the
 *   caller and die with M.  A level outside [0, levels): SPL_ERROR_argument_missing.
 * spl_amg_info: [0] n, [1] levels, [2] sum of nnz(A_l), [3] nnz(A_0), [4] coarsest n, [5] first tail level or -1,
 *   [6] bytes of device memory held, [7] flags (1 a zero diagonal was seen, 2 complex).
 *
 * spl_amg_apply_dev: x = cycle(0, b), a fixed linear operator:
 *     cycle(l, b):  x = w (.) b                                  (the first sweep from x = 0)
 *       coarsest:   (coarse_sweeps - 1) times  t = A_l x;  x = x + w (.) (b - t);           return x
 *       otherwise:  (nu - 1) times the same sweep
 *                   t = A_l x;  r = b - t;  b' = R r;  e = cycle(l + 1, b');  x = x + P e
 *                   nu times the sweep;                                                      return x
 *   Every entry-wise operation is one difference, one product (Data.Complex's on complex handles, w first) and one sum,
 *   each rounded once.  A_l x, R r and x + P e are spl_matrix_spmv_dev on the level handles in SPL_ORDER_REFERENCE, the
 *   last with `accumulate`: a * x + acc in ascending column order from +0.0 (from x_i when accumulating).  (An R of
 *   at most 16384 rows with 32 entries and more a row on average goes a wavefront a row instead: 64 products at a
 *   time, each rounded on its own, added in that same order whatever the row's length: the serial sum exactly, and
 *   the same bits as the SpMV for rows of up to 512 entries.)  The result is
 *   therefore a serial restatement's bit for bit, with the SpMV's caveat for rows of more than 512 entries, as in the
 *   Krylov section; SPL_ORDER_FREE on A voids the bits of level 0 only, in the way that section says.  The cycle is
 *   symmetric for a Hermitian A (equal pre- and post-sweeps, the first from zero, coarse Jacobi from zero), which is
 *   what CG needs.
 *   The tail: the levels from the first level l on such that l and every deeper level has n <= SPL_AMG_TAIL_ROWS (read
 *   by spl_amg_create; default 1024, 0 disables, larger values are clamped to 1024) and no row of A, P or R longer than
 *   512 entries.  Their whole sub-cycle, down and up, is ONE launch of ONE workgroup: a lane owns a row and walks its
 *   entries serially in ascending column order, so the bits are those of the launch-per-step path by construction; the
 *   vectors are M's work vectors, with workgroup barriers between the steps; nothing waits on another workgroup.
 *   Applications on one object are serialised under its lock, and one enqueued on another stream than the one before it
 *   waits for that one on the device.  The call enqueues on `stream` and does not synchronise.  d_b and d_x are DEVICE
 *   vectors of n entries (packed pairs on complex handles), d_b != d_x.  n == 0: SPL_OK.  Errors:
 *   SPL_ERROR_invalid_handle; SPL_ERROR_argument_missing (a NULL or misaligned pointer, or d_b == d_x).
 * spl_amg_apply: the same with HOST vectors, on the default stream; synchronises.
 * spl_krylov_set_preconditioner_amg: z = cycle(0, r) as the M^-1 of the Krylov section.  M is BORROWED and may serve
 *   several solvers.  It and spl_krylov_set_preconditioner exclude each other: each call clears what the other set;
 *   M == NULL clears.  spl_krylov_info's [2] gains flag 16.  The cycle's kernels do not read the solver's `done`: they
 *   write only z and M's own vectors, which nothing reads once `done` is set, so the protocol needs nothing from them.
 *   Errors: SPL_ERROR_invalid_handle (K, or M neither NULL nor an AMG object); SPL_ERROR_dimension_mismatch (another
 *   size, value kind or device). */
int spl_matrix_aggregate(void *H, uint64_t seed, int *d_agg, int *d_roots, int64_t info[8]);
int spl_amg_create(void *A, const int64_t opt[8], void **M);
int spl_amg_info(void *M, int64_t info[8]);
int spl_amg_level(void *M, int level, void **HA, void **HP, void **HR, const double **d_w, int64_t dims[2]);
int spl_amg_apply_dev(void *M, const double *d_b, double *d_x, void *stream);
int spl_amg_apply(void *M, const double *b, double *x);
void spl_amg_free(void **M);
int spl_krylov_set_preconditioner_amg(void *K, void *M);

/* ---- restarted GMRES on handles and the fused multi-vector inner product (csrc/gmres.hip) ------------------------------
 * spl_vector_dots_dev: d_out[i] = <V[:, i], w>, i = 0 ... k - 1, of n entries of value_width doubles each, all in DEVICE
 *   memory (complex: packed pairs, conjugate on the left).  Column i starts at d_V + i * ldv * value_width doubles,
 *   ldv >= n.  Each value is BIT FOR BIT what spl_vector_dot_dev(n, value_width, V[:, i], w, ...) writes: the same chunks
 *   of 4096, 256 lanes, halving tree and fold of partials; the order is a function of n alone, there is no floating-point
 *   atomic and no kernel waits for another workgroup, and SPL_KRYLOV_GRID does not show in the bits.  ONE pass computes
 *   all k: a workgroup loads its chunk of w once and streams the columns past it; the levels of the fold run on k *
 *   value_width planes at once.  Enqueued on `stream`, no synchronisation; the partials are a pool block per call.
 *   1 <= k <= 128; n == 0 writes +0.0 k times.  Errors, in this order: n < 0 SPL_ERROR_n_nonpositive; value_width not
 *   1 or 2, k outside 1 ... 128, ldv < n, a NULL pointer (d_V and d_w only when n > 0) or one that is not aligned to an
 *   entry: SPL_ERROR_argument_missing.
 *
 * spl_gmres_create: a solver object for the whole square handle A with restart length `restart`, 1 ... 128 (it may
 *   exceed n).  Ownership, borrowing, the lock (one solve at a time) and the error order are spl_krylov_create's;
 *   SPL_ERROR_argument_missing for a restart outside the range comes where "unknown method" comes there.  The object
 *   holds restart + 3 vectors (the basis v_0 ... v_restart, where slot j + 1 receives w before it is normalised, u and
 *   M^-1 u), the partials, the tables of a cycle (Hessenberg column / R, rotations, g, y) and a status block, all in
 *   device memory: info[3] has the bytes.  The operator is spl_matrix_spmv_dev as the caller configured it;
 *   SPL_ORDER_FREE voids the bit contract.
 * spl_gmres_set_preconditioner, spl_gmres_set_preconditioner_amg: as the spl_krylov_ calls; M^-1 is applied from the
 *   right.
 *
 * The method.  Every real operation is rounded once; a product of two entries is Data.Complex's, a real number times an
 * entry and an entry over a real number are done part by part; sqrt is IEEE's; threshold = max(rtol sqrt(Re<b,b>), atol)
 * and met(rho) means sqrt(rho) <= threshold, as above.
 *   cycle start:  r = b - A x  (first cycle with use_x0 == 0: r = b, x = 0, no product)
 *                 rho = Re<r,r>;  residual[0] = sqrt(rho);  first cycle: history[0] = residual[1] = sqrt(rho), <b,b>
 *                 rho or <b,b> not finite: reason 3;  met(rho): reason 0;  it == max_iter: reason 1
 *                 beta = sqrt(rho);  v_0 = r / beta;  g_0 = beta
 *   step j:       z = M^-1 v_j (no preconditioner: z IS v_j);  w = A z
 *                 c1_i = <v_i, w>, i = 0 ... j  (one pass);  w = ((w - c1_0 v_0) - c1_1 v_1) - ...  (ascending i)
 *                 c2_i = <v_i, w>;  w = w - sum c2_i v_i the same way;  h_i = c1_i + c2_i;  eta = sqrt(Re<w,w>)
 *                 an h_i or eta not finite: reason 3, the step is dropped and the cycle closes with k = j columns
 *                 i = 0 ... j-1:  (h_i, h_(i+1)) <- (conj(c_i) h_i + s_i h_(i+1),  c_i h_(i+1) - s_i h_i)
 *                 t = sqrt((Re h_j)^2 + (Im h_j)^2 + eta^2), left to right
 *                 t == 0: reason 2, the step is dropped, close with k = j;  t not finite: reason 3, likewise
 *                 c_j = h_j / t;  s_j = eta / t;  R_ij = h_i (i < j);  R_jj = t
 *                 g_(j+1) = -(s_j g_j);  g_j = conj(c_j) g_j;  it = it + 1;  history[it] = |g_(j+1)|
 *                 (sqrt(re^2 + im^2); real: the absolute value)
 *                 close with k = j + 1 when history[it] <= threshold, or eta == 0, or j + 1 == restart, or
 *                 it == max_iter;  otherwise v_(j+1) = w / eta and go on
 *   close:        k == 0: x unchanged.  Otherwise i = k-1 ... 0:  a = g_i;  a = a - R_il y_l, l = i+1 ... k-1 ascending;
 *                 y_i = a / R_ii;  u = y_0 v_0;  u = u + y_l v_l ascending;  x = x + M^-1 u (or + u)
 *                 residual[1] = history[it];  a reason set inside the cycle ends the solve here; otherwise: cycle start
 * s_j is real because the subdiagonal entry is a norm, and no rotation divides by |h_j|.  The estimate history[it] only
 * ENDS a cycle: reason 0 is decided at a cycle start alone, on the true residual of the x that is returned, so the last
 * cycle is sometimes a single step.
 *
 * spl_gmres_solve_dev: vectors, use_x0, rtol, atol, max_iter and the argument errors as spl_krylov_solve_dev, with
 *   `residual` NULL refused where `result` NULL is.  No scalar leaves the device during a cycle: the scalar work of a
 *   step and the back-substitution of a close are one launch of one workgroup each.  The host cannot know a cycle's
 *   length: it issues the launches of all `restart` steps and the close, and every kernel of a step returns without
 *   touching a vector once the cycle is closed or the solve is done.  The host reads the status block after every
 *   check_every-th cycle (0: every cycle); x, the counts, the history and the residuals do not depend on check_every,
 *   only the launches issued for nothing do.  No captured graph, no kernel that waits for another workgroup, no
 *   floating-point atomic.  result = {iterations, reason (as spl_krylov_solve_dev), cycles started, SpMVs issued,
 *   preconditioner applications issued, 0}; residual = {|b - A x| as the last cycle start computed it, the estimate at
 *   the last close}; history: NULL or max_iter + 1 doubles on the HOST.  n == 0: SPL_OK and zeros.  b = 0 without a
 *   start: x = 0, 0 iterations, reason 0.
 * spl_gmres_solve: the same with HOST vectors, on the default stream, a look after every cycle.
 * spl_gmres_info: [0] n, [1] restart, [2] flags as spl_krylov_info's (16: AMG), [3] bytes of device memory, [4] solves,
 *   [5] iterations of the last solve, [6] launches of the last solve, [7] 0.
 * spl_gmres_free: idempotent, as spl_krylov_free. */
int spl_vector_dots_dev(int64_t n, int value_width, int k, const double *d_V, int64_t ldv, const double *d_w, double *d_out,
                        void *stream);
int spl_gmres_create(void *A, int restart, void **G);
int spl_gmres_set_preconditioner(void *G, void *T1, const double *d_mid, void *T2);
int spl_gmres_set_preconditioner_amg(void *G, void *M);
int spl_gmres_solve_dev(void *G, const double *d_b, double *d_x, int use_x0, double rtol, double atol, int64_t max_iter,
                        int check_every, int64_t result[6], double *history, double residual[2], void *stream);
int spl_gmres_solve(void *G, const double *b, double *x, int use_x0, double rtol, double atol, int64_t max_iter,
                    int64_t result[6], double *history, double residual[2]);
int spl_gmres_info(void *G, int64_t info[8]);
void spl_gmres_free(void **G);

/* ---- a block of inner products in one pass (csrc/gram.hip) --------------------------------------------------------------
 * spl_vector_gram_dev: G[i][j] = <V[:, i], W[:, j]>, i = 0 ... k - 1, j = 0 ... l - 1, of n entries of value_width
 *   doubles each, all in DEVICE memory (complex: packed pairs, conjugate on the left).  V and W are column blocks in the
 *   layout of spl_vector_dots_dev: column i of V at d_V + i * ldv * value_width doubles, ldv >= n, column j of W at
 *   d_W + j * ldw * value_width, ldw >= n; they may be the same block.  G is column major, entry (i, j) at
 *   d_G + (j * ldg + i) * value_width doubles, ldg >= k.  upper == 1 writes only the entries with i <= j and leaves the
 *   rest of G untouched (the Hermitian use, V == W: the caller mirrors with conjugates); the gaps of a padded ldg are
 *   never written.  Every entry is BIT FOR BIT what spl_vector_dot_dev(n, value_width, V[:, i], W[:, j], ...) writes:
 *   the same chunks of 4096, lane t of 256 adding its 16 products in ascending order from +0.0, the halving tree and
 *   the fold of partials, every product rounded on its own; no floating-point atomic, and no kernel waits for another
 *   workgroup.  What makes it one pass: a workgroup takes a chunk and a tile of columns of W, each lane keeps its 16
 *   entries of those columns in registers and the columns of V stream past them, so V is read once per tile and not
 *   once per column of W.  The tile (SPL_GRAM_TILE = 1, 2 or 4 columns of W, for measurement; default 4 real, 2
 *   complex), SPL_KRYLOV_GRID and the placement of workgroups do not show in the bits.  The partials are a pool block
 *   per call; a call whose partials would exceed 64 MiB is cut into blocks of columns inside the entry point, so the
 *   scratch is at most max(64 MiB, n / 16 bytes) plus one middle level.  (SPL_GRAM_SCRATCH = bytes is a TEST HOOK and
 *   no tuning knob: it replaces the 64 MiB by any positive number, down to 1, so that the tests reach the cut at a few
 *   thousand rows; it does not show in the bits either.)  Enqueued on `stream`, no synchronisation.
 *   1 <= k, l <= 128; n == 0 writes +0.0 to every entry it would write.  Errors, in this order: n < 0
 *   SPL_ERROR_n_nonpositive; value_width not 1 or 2; k or l outside 1 ... 128, upper not 0 or 1, ldv < n, ldw < n,
 *   ldg < k; a NULL pointer (d_V and d_W only when n > 0); a pointer not aligned to an entry; G overlapping V or W
 *   (n > 0): SPL_ERROR_argument_missing. */
int spl_vector_gram_dev(int64_t n, int value_width, int k, int l, const double *d_V, int64_t ldv, const double *d_W,
                        int64_t ldw, double *d_G, int64_t ldg, int upper, void *stream);

/* ---- thick-restart Lanczos on handles and the in-place basis rotation (csrc/eigsh.hip) ---------------------------------
 * A few eigenpairs of a real symmetric or complex Hermitian handle without a factorisation: restarted Lanczos with full
 * reorthogonalisation and thick restarts (Wu & Simon's TRLan scheme), directly on A for the ends of the spectrum, or on
 * (A - sigma I)^-1 through a spl_krylov object for the eigenvalues nearest sigma.  The contract is the one of the
 * sections above: values, vectors, residuals, history and counts are a serial restatement's bit for bit.
 *
 * spl_vector_rotate_dev: column i of the result, i = 0 ... k - 1, is x = Y[0][i] v_0; x = x + Y[l][i] v_l for
 *   l = 1 ... m - 1 ascending, where v_l is column l of V (n entries of value_width doubles, complex as packed pairs,
 *   column l at d_V + l * ldv * value_width doubles, ldv >= n: the layout of spl_vector_dots_dev) and Y is a REAL m x k
 *   matrix in DEVICE memory, column major, Y[l][i] at d_Y[i * ldy + l], ldy >= m.  A real number times an entry is done
 *   part by part; each term is one product and one sum, each rounded once.  1 <= k <= m <= 128.  d_out == NULL: the
 *   result overwrites V[:, 0:k] IN PLACE (no second basis is allocated; columns k ... m - 1 and the rows from n on are
 *   untouched); otherwise it goes to d_out (column i at d_out + i * ldo * value_width, ldo >= n), V is untouched and
 *   d_out may not overlap V.  V is read once and the k columns are written once: a workgroup stages a tile of rows in
 *   LDS, so every input of a row is read before any output of that row is written.  No floating-point atomic, no
 *   kernel waits for another workgroup; the tile height (SPL_EIGSH_ROTATE_ROWS = 16, 32 or 64, for measurement) and
 *   SPL_KRYLOV_GRID do not show in the bits.  Enqueued on `stream`, no synchronisation.  n == 0: SPL_OK, nothing is
 *   written.  Errors, in this order: n < 0 SPL_ERROR_n_nonpositive; value_width not 1 or 2, m outside 1 ... 128, k
 *   outside 1 ... m, ldv < n, ldy < m, ldo < n (with d_out), a NULL d_V or d_Y when n > 0, a pointer not aligned to an
 *   entry (d_Y: to a double), d_out overlapping V: SPL_ERROR_argument_missing.
 *
 * spl_eigsh_create: a solver object for the whole square handle A with a basis of ncv columns, 2 ... 128.  Ownership,
 *   borrowing, the lock (one solve at a time), the magic word and spl_eigsh_free's idempotence are spl_gmres_create's.
 *   Errors, in this order: SPL_ERROR_invalid_handle (A is no matrix handle); SPL_ERROR_argument_missing (E is NULL;
 *   otherwise *E = NULL first; then ncv outside 2 ... 128); SPL_ERROR_dimension_mismatch (not square);
 *   SPL_ERROR_invalid_matrix (a row-block handle); SPL_ERROR_device without a GPU; SPL_ERROR_invalid_matrix (a handle for
 *   which spl_matrix_hermitian says 0, or on which it cannot run: the test is a kernel, so it comes behind the device).
 *   The object holds ncv + 2 vectors (the basis v_0 ... v_ncv, where slot j + 1 receives w before it is normalised, and
 *   one product for the residuals), the partials, 7 ncv + ncv^2 doubles of tables (the coefficients of the two passes,
 *   alpha, beta, the residuals, Y) and a status block in device memory: info[3] has the bytes.  The operator is
 *   spl_matrix_spmv_dev as the caller configured it; SPL_ORDER_FREE voids the bit contract.
 * spl_eigsh_set_inverse: the operator becomes OP = (A - sigma I)^-1, applied as spl_krylov_solve_dev(K, v, w, use_x0 = 0,
 *   rtol, atol, max_iter) with the default check interval.  K is a spl_krylov object the CALLER built on A - sigma I
 *   (spl_matrix_lin) with whatever preconditioner they set; it is borrowed.  K == NULL: back to direct mode, the other
 *   arguments are not looked at.  Errors, in this order: SPL_ERROR_invalid_handle (E, or K, is no such object);
 *   SPL_ERROR_dimension_mismatch (K of another size, value kind or device); SPL_ERROR_n_nonpositive (max_iter < 0);
 *   SPL_ERROR_argument_missing (rtol or atol negative or NaN, sigma not finite).
 *
 * The method.  Every real operation is rounded once; a real number times an entry and an entry over a real number are
 * done part by part; <a,b> and its fold are those of the sections above.  OP v is spl_matrix_spmv_dev on A, or the
 * solve above; in inverse mode a solve whose reason is not 0 ends everything with reason 4 and no pairs.
 *   start:    eta = sqrt(Re<v0,v0>);  history[0] = eta;  eta not finite: reason 3, no pairs;  eta == 0: reason 2, no
 *             pairs;  v_0 = v0 / eta;  k = 0;  cycle = 0
 *   step j    (j = k ... ncv - 1):  w = OP v_j
 *             c1_i = <v_i, w>, i = 0 ... j  (one pass);  w = ((w - c1_0 v_0) - c1_1 v_1) - ...  (ascending i)
 *             c2_i = <v_i, w>;  w = w - sum c2_i v_i the same way
 *             alpha_j = Re(c1_j + c2_j);  beta_j = eta = sqrt(Re<w,w>);  ops = ops + 1
 *             alpha_j or eta not finite: reason 3, no pairs
 *             eta == 0: the cycle closes with m' = j + 1 and the solve ends behind the close
 *             otherwise v_(j+1) = w / eta;  behind step ncv - 1 the cycle closes with m' = ncv
 *   close:    T, real symmetric m' x m':  T_ii = theta_i and T_ik = T_ki = s_i for i < k (kept from the restart);
 *             T_jj = alpha_j for j >= k;  T_(j,j+1) = T_(j+1,j) = beta_j for k <= j < m' - 1;  beta_last = beta_(m'-1)
 *             T = Y diag(theta) Y^T by cyclic Jacobi on full symmetric storage, Y = I at the start:
 *               a sweep starts only if some strict upper entry is non-zero; in a sweep p ascending, q > p ascending,
 *               a = T_pq:  a == 0: skip;  |T_pp| + |a| == |T_pp| and |T_qq| + |a| == |T_qq|: T_pq = T_qp = 0, no rotation
 *               otherwise tau = (T_qq - T_pp) / (2 a);  t = sgn(tau) / (|tau| + sqrt(1 + tau tau)), sgn(0) = +1;
 *               c = 1 / sqrt(1 + t t);  s = t c;  for r != p, q:  (T_rp, T_rq) <- (c T_rp - s T_rq, s T_rp + c T_rq),
 *               mirrored;  T_pp = T_pp - t a;  T_qq = T_qq + t a (the old diagonal);  T_pq = T_qp = 0;  for all r:
 *               (Y_rp, Y_rq) <- (c Y_rp - s Y_rq, s Y_rp + c Y_rq)
 *               a 61st sweep, or a theta or an entry of Y not finite at the end: reason 3, no pairs
 *             cycle = cycle + 1;  the pairs are ordered stably by `which` (ties: lower column first), applied to the
 *             OPERATOR's theta:  0 largest algebraic, 1 smallest algebraic, 2 largest magnitude
 *             est_i = |beta_last Y[m'-1][i]|;  pairs = min(nev, m');  history[cycle] = max est_i, i < pairs
 *             pair i is converged when est_i <= max(tol |theta_i|, atol)
 *             eta was 0: reason 0 when m' >= nev, otherwise reason 2, with `pairs` pairs
 *             else all nev converged: reason 0;  else cycle == max_restarts: reason 1, the nev Ritz pairs are returned
 *             else restart:  k = min(m' - 1, nev + (m' - nev) / 2) (integer division);  V[:, :k] <- V Y[:, :k] in place
 *             by spl_vector_rotate_dev's kernel;  v_k <- v_(m');  theta_i is kept, s_i = beta_last Y[m'-1][i]
 *   finish:   X = V Y[:, :pairs] by the same kernel into d_vectors, not renormalised
 *             values[i] = theta_i, in inverse mode sigma + 1 / theta_i (IEEE)
 *             residuals[i] = sqrt(Re<r,r>), r = A x_i - values[i] x_i:  the product by spl_matrix_spmv_dev on A itself
 *             in both modes, each entry of r one product part by part and one difference
 * The test that drops a coupling is on |a| itself: on |t a| it drops couplings that still carry the last row of Y, and
 * the estimate becomes 0 on a residual that is not.  A single-vector Lanczos finds ONE copy of a multiple eigenvalue.
 *
 * spl_eigsh_solve_dev: d_v0 (n entries) and d_vectors (nev columns, ldx >= n entries apart) are DEVICE arrays; values,
 *   residuals (nev doubles each), result and history (NULL, or max_restarts + 1 doubles) are the HOST's.  d_v0 is
 *   required: the library draws no random numbers.  In direct mode no scalar leaves the device inside a cycle: one
 *   workgroup behind the folds writes alpha_j and beta_j into a table, the host issues every step of the cycle and each
 *   kernel returns once the cycle is closed; the close is the host's, ONE synchronisation per cycle.  In inverse mode
 *   the inner solve synchronises, and the status block is read behind every step.  No captured graph.
 *   result = {reason, cycles closed, applications of OP (a failed inner solve is not counted), pairs returned, inner
 *   iterations in total, most Jacobi sweeps of a close}; reasons: 0 converged, 1 max_restarts, 2 invariant subspace
 *   smaller than nev (or a zero start), 3 not finite, 4 inner solve failed.  Only the first result[3] entries of values,
 *   residuals and d_vectors are written.  Returns SPL_OK whenever it ran.  Errors, in this order:
 *   SPL_ERROR_invalid_handle (E); SPL_ERROR_argument_missing (values, residuals or result NULL);
 *   SPL_ERROR_n_nonpositive (max_restarts < 1); SPL_ERROR_argument_missing (not 1 <= nev < ncv <= n, `which` outside
 *   0 ... 2, tol or atol negative or NaN); SPL_ERROR_index_overflow (a history of 2^31 entries or more);
 *   SPL_ERROR_argument_missing (d_v0 or d_vectors NULL or not aligned to an entry, ldx < n).
 * spl_eigsh_solve: the same with a HOST v0 and HOST vectors, on the default stream.
 * spl_eigsh_info: [0] n, [1] ncv, [2] flags (1 complex, 2 inverse mode), [3] bytes of device memory, [4] solves,
 *   [5] cycles of the last solve, [6] launches of the last solve (the SpMV counted as one, inner solves not counted),
 *   [7] 0.
 * spl_eigsh_free: idempotent, as spl_krylov_free.
 *
 * spl_vector_rotate_z_dev: spl_vector_rotate_dev with a COMPLEX Y, for a block method's projected matrix on a complex
 *   Hermitian handle.  value_width must be 2.  Y is m x k packed pairs in DEVICE memory, column major, Y[l][i] at
 *   d_Y + 2 * (i * ldy + l) doubles, ldy >= m.  Column i of the result is x = Y[0][i] v_0; x = x + Y[l][i] v_l for
 *   l = 1 ... m - 1 ascending, where the product of Y[l][i] = a + b i and an entry c + d i is Data.Complex's,
 *   (a c - b d, a d + b c): four products, one difference and one sum, each rounded once; then one sum per part.
 *   Everything else is spl_vector_rotate_dev's: the in-place guarantee with d_out == NULL, the tile in LDS, the knobs
 *   that do not show, n == 0, and the errors in the same order, with "value_width not 2" where "not 1 or 2" comes there.
 *   spl_vector_rotate_dev itself is unchanged. */
#define SPL_EIGSH_largest_algebraic 0
#define SPL_EIGSH_smallest_algebraic 1
#define SPL_EIGSH_largest_magnitude 2
int spl_vector_rotate_dev(int64_t n, int value_width, int m, int k, double *d_V, int64_t ldv, const double *d_Y, int ldy,
                          double *d_out, int64_t ldo, void *stream);
int spl_vector_rotate_z_dev(int64_t n, int value_width, int m, int k, double *d_V, int64_t ldv, const double *d_Y, int ldy,
                            double *d_out, int64_t ldo, void *stream);
int spl_eigsh_create(void *A, int ncv, void **E);
int spl_eigsh_set_inverse(void *E, void *K, double sigma, double rtol, double atol, int64_t max_iter);
int spl_eigsh_solve_dev(void *E, int nev, int which, double tol, double atol, int64_t max_restarts, const double *d_v0,
                        double *values, double *d_vectors, int64_t ldx, double *residuals, int64_t result[6],
                        double *history, void *stream);
int spl_eigsh_solve(void *E, int nev, int which, double tol, double atol, int64_t max_restarts, const double *v0,
                    double *values, double *vectors, int64_t ldx, double *residuals, int64_t result[6], double *history);
int spl_eigsh_info(void *E, int64_t info[8]);
void spl_eigsh_free(void **E);

/* ---- LOBPCG on handles (csrc/lobpcg.hip, csrc/ritz_jacobi.hpp) -----------------------------------------------------------
 * A few extreme eigenpairs of a real symmetric or complex Hermitian handle by a BLOCK method with the preconditioner
 * inside the iteration (Knyazev's LOBPCG on an orthonormal basis): it finds every copy of a multiple eigenvalue that its
 * block has room for, and on the small end of an elliptic operator it applies one preconditioner cycle per column and
 * iteration instead of an inner solve.  The contract is the one of the sections above: values, vectors, residuals,
 * history and every count are a serial restatement's bit for bit, whatever SPL_KRYLOV_GRID, SPL_GMRES_DOTS_BATCH,
 * SPL_EIGSH_ROTATE_ROWS and SPL_GRAM_TILE are; SPL_ORDER_FREE on the operator voids it.  No captured graph, no
 * floating-point atomic, no kernel waits for another workgroup.
 *
 * spl_lobpcg_create: a solver object for the whole square handle A with a block of `block` columns, 1 ... 42 (so that
 *   the basis of 3 block columns stays within the 128 of spl_vector_gram_dev and spl_vector_rotate_dev).  Ownership,
 *   borrowing, the lock (one solve at a time) and spl_lobpcg_free's idempotence are spl_eigsh_create's, and so are the
 *   errors and their order, with "block outside 1 ... 42" where "ncv outside 2 ... 128" comes there.  The object holds
 *   7 block + 1 vectors (S = [X | P | W], A S, R for the preconditioner, one product for the residuals at the end), the
 *   partials, 30 block^2 + 19 block doubles and 3 block ints of tables (T, the rotation, the coefficients of the two
 *   passes, norms, residuals, flags) and a status block in device memory: info[3] has the bytes.  The products are
 *   spl_matrix_spmv_many_dev's (the CSR image, reference order), the one of the residuals at the end
 *   spl_matrix_spmv_dev's.
 * spl_lobpcg_set_preconditioner, spl_lobpcg_set_preconditioner_amg: as the spl_krylov_ calls; w = M^-1 r is applied
 *   column by column.
 *
 * The method.  b = block; S has the columns s_0 ... s_(3b-1): X = s_0 .. s_(b-1), P the next b, W the last b; A S is kept
 * beside it.  Every real operation is rounded once; a real number times an entry and an entry over a real number are done
 * part by part; <a,b> and its fold are those of the sections above; the product of two complex numbers is Data.Complex's.
 *   settle(c): column c against the c columns before it.  eta0 = sqrt(Re<s_c,s_c>);  c > 0:  c1_i = <s_i, s_c>, i < c
 *             (one pass);  s_c = ((s_c - c1_0 s_0) - c1_1 s_1) - ... ascending;  c2_i = <s_i, s_c>;  s_c = s_c - sum c2_i
 *             s_i the same way;  eta2 = sqrt(Re<s_c,s_c>)  (c == 0: eta2 is eta0 computed again)
 *             eta0 or eta2 not finite: flag_c = 2;  else eta2 == 0 or eta2 <= 2^-40 eta0: flag_c = 1 (dropped);  else
 *             flag_c = 0.  flag_c != 0: s_c = 0 (every entry +0.0);  else s_c = s_c / eta2.  The decision is taken on the
 *             device; a zero column gives +0.0 coefficients and terms, so the launches do not depend on what dropped.
 *             2^-40: what is left of a column after the first pass is below 2^-40 of it exactly when the second pass can
 *             no longer restore orthogonality to rounding level from it.
 *   close(m, k): G_ij = <s_i, (A s)_j> for i <= j < m by spl_vector_gram_dev's kernel (upper).
 *             A flag_j == 2 with j < m, or any flag other than 0 on a column of X (j < b): reason 3.
 *             kept = the j < m with flag_j == 0, ascending, m' of them.
 *             T (m' x m'):  T_aa = Re G_(kept a, kept a);  T_ac = G_(kept a, kept c) and T_ca its conjugate for a < c;
 *             an entry of T not finite: reason 3.
 *             T = Y diag(theta) Y^H by cyclic Jacobi with Y = I at the start: real handles by the rule of the Lanczos
 *             section; complex handles by the same rule with the coupling turned real first:
 *               a sweep starts only if some strict upper entry has a non-zero part; p ascending, q > p ascending,
 *               a = T_pq:  both parts 0: skip;  g = sqrt(Re a Re a + Im a Im a);  |T_pp| + g == |T_pp| and
 *               |T_qq| + g == |T_qq|:  T_pq = T_qp = 0, no rotation;  otherwise u = (Re a / g, Im a / g);
 *               tau = (T_qq - T_pp) / (2 g);  t, c, s from tau as in the real rule;  for r != p, q:  z = T_rq conj(u)
 *               = (Re T_rq Re u + Im T_rq Im u,  Im T_rq Re u - Re T_rq Im u);  (T_rp, T_rq) <- (c T_rp - s z,
 *               s T_rp + c z) part by part, T_pr and T_qr their conjugates;  T_pp = T_pp - t g;  T_qq = T_qq + t g (the old
 *               diagonal);  T_pq = T_qp = 0;  for all r:  z = Y_rq conj(u) likewise;  (Y_rp, Y_rq) <- (c Y_rp - s z,
 *               s Y_rp + c z).  A 61st sweep, or a theta or a part of Y not finite at the end: reason 3.
 *             The pairs are ordered stably by `which` (ties: lower column first).  Z (m x k):  column i < b has
 *             Y[a][order i] in row kept_a and +0.0 in the rows of flagged columns;  column b + i (when k = 2 b) is column
 *             i with the rows 0 ... b-1 set to +0.0.  S[:, :k] <- S[:, :m] Z and (A S)[:, :k] <- (A S)[:, :m] Z in place
 *             by spl_vector_rotate_dev's kernel (complex handles: spl_vector_rotate_z_dev's);  theta_i = theta_(order i),
 *             i < b.  Then X' is settled again, settle(0) ... settle(b-1), and A X' with it:  (A s)_c = ((A s)_c - c1_0
 *             (A s)_0) - ... and the same with c2, ascending, then (A s)_c / eta2, or zeros where s_c got them: A X' stays
 *             the product of X'.  (The rotation alone leaves X' orthonormal to ITS rounding, and the loss adds up: 1.2e-13
 *             after 56 iterations on a 12 x 12 grid, which biases theta by as much.)  A flag on a column of X is found at
 *             the next close: reason 3.
 *   start:    X = X0;  P = 0 (flagged as dropped, not counted);  settle(0) ... settle(b-1);  a flag 2: reason 3, no pairs;
 *             a flag 1: reason 2, no pairs (the start block is rank deficient).  A X by one product of b columns;
 *             close(b, b).
 *   iteration it = 0, 1, ...:
 *             r_i = (A x)_i - theta_i x_i, i < b, each entry one product part by part and one difference;
 *             rho_i = sqrt(Re<r_i,r_i>);  a rho_i not finite: reason 3, no pairs.  history[it] = max rho_i, i < nev.
 *             Column i < nev is converged when rho_i <= max(tol |theta_i|, atol);  all nev converged: reason 0;  else
 *             it == max_iter: reason 1;  both end at `finish`.
 *             w_i = M^-1 r_i, or r_i without a preconditioner, into column 2 b + i.
 *             settle(b) ... settle(3 b - 1): P and then W against everything before them.  A [P | W] by ONE product of
 *             2 b columns (a zero column gives a zero column).  close(3 b, 2 b): [X' | P'] and [A X' | .].  Flags 1 are
 *             counted as drops, those of P in iteration 0 excepted.  iterations = it + 1.
 *   finish:   d_vectors = the first nev columns of X as the last close left them;
 *             values[i] = theta_i;  residuals[i] = sqrt(Re<r,r>), r = A x_i - theta_i x_i with a fresh
 *             spl_matrix_spmv_dev product.
 * Limits: converged columns are not locked (they stay in the block and are iterated on); interior eigenvalues,
 * row-block handles and several devices are not served.
 *
 * The generalized problem A x = lambda B x.  spl_lobpcg_set_mass gives the object a Hermitian positive definite handle B
 *   (a FEM mass matrix); B is borrowed, as A is.  No solve with B is needed: the method above runs in the inner product
 *   <u,v>_B = <u, B v>, with B S kept beside S and A S, so the Ritz problem stays a standard one.  The object then holds
 *   10 block + 2 vectors (B S: 3 block; a second product for the residuals at the end); info[2] has bit 32, info[3] the
 *   bytes, info[7] the columns multiplied by B in the last solve (result[2] stays A's).  B == NULL returns the object
 *   to the standard method, releases that memory, and info[3] has its old value again.  Positive definiteness is the
 *   caller's promise and is not tested.  Errors, in this order: SPL_ERROR_invalid_handle (L is no such object, or B is
 *   no matrix handle); SPL_ERROR_dimension_mismatch (B is not n x n, of the other value kind, or on another device);
 *   SPL_ERROR_invalid_matrix (B is a row block, or spl_matrix_hermitian says 0).
 *   The method with B: everything not named here is the text above unchanged.
 *   settle(c): q0 = Re<s_c, (B s)_c>;  c > 0:  c1_i = <(B s)_i, s_c>, i < c (one pass, B S as the basis);  s_c and (B s)_c
 *             are updated TOGETHER with c1, ascending, a product and a difference per term (spl_vector_update_pair_dev's
 *             kernel);  c2_i likewise, and the paired update with c2, which delivers q2 = Re<s_c, (B s)_c>  (c == 0: q2
 *             is q0 computed again).  q0 or q2 not finite: flag_c = 2;  else q0 < 0 or q2 < 0: flag_c = 1;  else
 *             eta0 = sqrt(q0), eta2 = sqrt(q2), eta2 == 0 or eta2 <= 2^-40 eta0: flag_c = 1;  else flag_c = 0.
 *             flag_c != 0: s_c and (B s)_c become +0.0;  else both are divided by eta2.
 *   settle of X' after a close: (A s)_c receives the same coefficients, the division and the zeros, as above.
 *   close(m, k): G = S^H (A S), upper, unchanged; the rotation is applied in place to S, A S and B S.
 *   start:    X = X0;  B X by one product of b columns (spl_matrix_spmv_many_dev on B);  settle(0) ... settle(b-1), the
 *             flags as above;  A X by one product;  close(b, b).
 *   iteration: r_i = (A x)_i - theta_i (B x)_i, one product part by part and one difference per entry;  rho_i =
 *             sqrt(Re<r_i,r_i>), the Euclidean norm; the convergence rule is unchanged.  w_i = M^-1 r_i into column
 *             2 b + i;  B W by one product of b columns into (B S)[:, 2b:3b] (P's image is the rotation's);
 *             settle(b) ... settle(3 b - 1);  A [P | W] by one product of 2 b columns;  close(3 b, 2 b).
 *   finish:   values[i] = theta_i;  residuals[i] = |A x_i - theta_i B x_i|_2 from fresh spl_matrix_spmv_dev products
 *             on A and on B.  The vectors are B-orthonormal.
 *   With B an identity handle every quantity equals the standard method's bit for bit, but for the sign of a zero that
 *   an identity product may turn positive.  Two synchronisations per iteration, as above; the launch sequence does not
 *   depend on what dropped.  Lanczos (spl_eigsh_*) takes no mass matrix; a B that is not definite is not served.
 *
 * spl_vector_update_pair_dev: w = ((w - c_0 v_0) - c_1 v_1) - ... and bw = ((bw - c_0 (Bv)_0) - c_1 (Bv)_1) - ... over
 *   the k columns of V and BV (laid out as in spl_vector_dots_dev, ldv, ldbv >= n), ascending, with the same k
 *   coefficients d_coef (device memory) for both, in ONE launch: each term is one product (Data.Complex's on packed
 *   pairs) and one difference.  With d_q given, *d_q = Re<w, bw> of the results, the real part of what
 *   spl_vector_dot_dev(n, value_width, w, bw, ...) writes bit for bit; SPL_KRYLOV_GRID does not show in the bits.
 *   1 <= k <= 128; n == 0 returns SPL_OK and +0.0 goes to d_q.  Enqueues on `stream`, no synchronisation.  Errors, in
 *   this order: SPL_ERROR_n_nonpositive (n < 0); SPL_ERROR_argument_missing (value_width not 1 or 2, k out of range,
 *   ldv < n or ldbv < n; a NULL pointer other than d_q, the vector pointers only when n > 0; a pointer not aligned to an
 *   entry; w or bw overlapping each other, V or BV).
 *
 * spl_lobpcg_solve_dev: d_X0 (block columns, ldx0 >= n entries apart) and d_vectors (nev columns, ldx >= n apart) are
 *   DEVICE arrays; values, residuals (nev doubles each), result and history (NULL, or max_iter + 1 doubles) are the
 *   HOST's.  d_X0 is required and is not changed: the library draws no random numbers.  `which` is
 *   SPL_EIGSH_smallest_algebraic or SPL_EIGSH_largest_algebraic.  The host synchronises twice per iteration (the
 *   residual norms; T and the flags), once at the start and once at the end.  result = {reason, iterations, columns
 *   multiplied by A, pairs returned, preconditioner applications, most Jacobi sweeps of a close, columns dropped in
 *   total, synchronisations}; reasons: 0 converged, 1 max_iter, 2 start block rank deficient, 3 not finite.  Reasons 0
 *   and 1 return nev pairs, 2 and 3 none, and only the first result[3] entries of values, residuals and d_vectors are
 *   written.  Returns SPL_OK whenever it ran.  Errors, in this order: SPL_ERROR_invalid_handle (L);
 *   SPL_ERROR_argument_missing (values, residuals or result NULL); SPL_ERROR_n_nonpositive (max_iter < 0);
 *   SPL_ERROR_argument_missing (not 1 <= nev <= block <= n, `which` largest magnitude or unknown, tol or atol negative
 *   or NaN); SPL_ERROR_index_overflow (a history of 2^31 entries or more); SPL_ERROR_argument_missing (d_X0 or d_vectors
 *   NULL, ldx0 < n, ldx < n, a pointer not aligned to an entry).
 * spl_lobpcg_solve: the same with a HOST X0 and HOST vectors, on the default stream.
 * spl_lobpcg_info: [0] n, [1] block, [2] flags (1 complex, and 2 / 4 / 8 / 16 as spl_krylov_info's), [3] bytes of device
 *   memory, [4] solves, [5] iterations of the last solve, [6] launches of the last solve (a product counted as
 *   one, a Gram matrix as the kernels it enqueues, whatever its cut), [7] 0 (with a mass matrix: see below).
 * spl_lobpcg_free: idempotent, as spl_krylov_free. */
int spl_lobpcg_create(void *A, int block, void **L);
int spl_lobpcg_set_preconditioner(void *L, void *T1, const double *d_mid, void *T2);
int spl_lobpcg_set_preconditioner_amg(void *L, void *M);
int spl_lobpcg_solve_dev(void *L, int nev, int which, double tol, double atol, int64_t max_iter, const double *d_X0,
                         int64_t ldx0, double *values, double *d_vectors, int64_t ldx, double *residuals,
                         int64_t result[8], double *history, void *stream);
int spl_lobpcg_solve(void *L, int nev, int which, double tol, double atol, int64_t max_iter, const double *X0,
                     int64_t ldx0, double *values, double *vectors, int64_t ldx, double *residuals, int64_t result[8],
                     double *history);
int spl_lobpcg_info(void *L, int64_t info[8]);
void spl_lobpcg_free(void **L);
int spl_lobpcg_set_mass(void *L, void *B);
int spl_vector_update_pair_dev(int64_t n, int value_width, int k, const double *d_V, int64_t ldv, const double *d_BV,
                               int64_t ldbv, const double *d_coef, double *d_w, double *d_bw, double *d_q, void *stream);

/* select a kernel variant for spl_matrix_spmv_dev (tuning / ablation only): 0 = default
 * (whatever spl_matrix_optimize chose), 1-6 CSR-stream shapes, 7 sub-wavefront kernel, 8
 * column-blocked image, 9-11 gather cache policies, 15 sliced-ELL image, 16 column-sorted panel
 * image (order-free sums, see spl_matrix_set_spmv_order); 12-14 are timing-only
 * ablations that do not compute A x and are refused unless SPL_ALLOW_ABLATION=1.
 * Returns SPL_ERROR_argument_missing for an unknown or refused variant. */
int spl_matrix_set_variant(void *H, int variant);

/* Analyse the matrix once (like umfpack_*_symbolic) and build the image variant 0 then uses:
 * the column-blocked image when columns have no locality and x exceeds the L2s
 * (csrc/spmv_blocked.hip), the sliced-ELL image for regular rows with locality
 * (csrc/spmv_sell.hip), or nothing (CSR-stream kernel).  Results are bit-identical either way.
 * After spl_matrix_set_spmv_order(H, SPL_ORDER_FREE) the column-sorted panel image (csrc/spmv_panel.hip) takes
 * the place of the column-blocked one where it pays; its two launch parameters are then timed against their
 * neighbours on a scratch vector (about a hundred launches, once) and the fastest pair kept. */
int spl_matrix_optimize(void *H);
/* build that image with an explicit shape (tuning / ablation): panels of rows_per_panel rows,
 * column blocks of 2^cols_log2 columns (rows_per_panel << cols_log2 must fit 31 bits);
 * 0,0 = choose.  unroll: 0 default, {4,8,10,12} 64-entry chunks per register set of the
 * lockstep kernel; negative {-1,-2,-4,-8} selects the free-running baseline kernel. */
int spl_matrix_build_blocked(void *H, int rows_per_panel, int cols_log2, int unroll);

/* Order of the floating-point sums of spl_matrix_spmv_dev / mulv / gaxpy on this handle.
 * The CONTRACT of both modes is north_star's: every value within 1e-10 relative of the reference's.
 * SPL_ORDER_REFERENCE (default): every y[r] receives a*x + y in ascending column order, each
 * multiply and add separately rounded — the evaluation order of axpy_ (Sparse.hs:447-451).  On gfx950
 * this reproduces the reference's bits, run after run (what the parity tests check), with two caveats that
 * keep bit-identity an observation rather than a promise: the column-blocked kernel relies on same-address
 * lanes of one LDS atomic being applied in lane order (pinned by tests/test_gpu_spmv_blocked.py, not by an
 * ISA document), and the CSR-stream kernel sums a row longer than one 512-entry chunk with a wavefront tree.
 * SPL_ORDER_FREE: the products of a row may be added in any order (still separately rounded
 * multiplies and adds): results agree with the reference to rounding level (1e-10 relative is
 * north_star's contract; observed ~1e-16) but need not be bit-identical, nor identical from run to
 * run.  Lets spl_matrix_optimize use the column-sorted panel image (csrc/spmv_panel.hip), which
 * sends about a quarter fewer requests to the L2 on matrices without column locality. */
#define SPL_ORDER_REFERENCE 0
#define SPL_ORDER_FREE 1
int spl_matrix_set_spmv_order(void *H, int order);
/* CUs to leave free for a kernel that runs beside the SpMV (the collective of a multi-GPU step): the images
 * spl_matrix_optimize / _build_* lay out afterwards have one panel (group) per remaining CU when the row block
 * takes one generation, so the persistent grid is that much smaller.  Call before spl_matrix_optimize.
 * Default 0, or the environment variable SPL_SPMV_RESERVED_CUS. */
int spl_matrix_set_reserved_cus(void *H, int reserved);
/* Diagnostics only: `blocks` workgroups of `threads` threads copy d_buf (count doubles) onto itself for
 * `milliseconds` (at most 2000) on `stream` — a stand-in for a collective's channel kernels when measuring what
 * reserved CUs are worth on one GPU (tools/bench_reserved_cus.py). */
int spl_debug_occupy(int blocks, int threads, double milliseconds, double *d_buf, size_t count, void *stream);
/* diagnostics / tests: the library's own radix sort (csrc/radix_sort.hip; the nested dissection orders its level
 * structures with it) on d_keys[0 .. n) in device memory, in place, ascending by the low nbits bits of the keys */
int spl_debug_sort_u64(unsigned long long *d_keys, long long n, int nbits, void *stream);
/* build the column-sorted panel image with an explicit shape (tuning / ablation): panels of
 * rows_per_panel rows (<= 20479: one workgroup's LDS), index blocks of 2^cols_log2 columns
 * (<= 17); 0,0 = choose.  `form` says which kernel walks the image, `unroll` how deep its pipeline is:
 *   form                       kernel                                                    unroll (0 = default)
 *   SPL_PANEL_FORM_DEFAULT     paired, 2 index blocks per phase when cols_log2 = 17,     as for the paired forms; with
 *                              else 1                                                    0,0,0,0 on a large matrix the
 *                                                                                        build times the neighbours,
 *                                                                                        the rounds form among them
 *   SPL_PANEL_FORM_CHUNK_K1    one 64-entry chunk per load instruction, 1 / 2 index      chunks per wavefront and
 *   SPL_PANEL_FORM_CHUNK_K2    blocks per barrier phase                                  register set: 4, 6, 8, 10, 12
 *                                                                                        (0: from the mean phase)
 *   SPL_PANEL_FORM_PAIRED_K1   paired storage (two chunks per 8-byte key / 16-byte       pairs per wavefront and register
 *   SPL_PANEL_FORM_PAIRED_K2   value load), 1 / 2 index blocks per phase; the only       set: 2 ... 4 (K1), 3 ... 6 (K2)
 *                              forms that take column slices (SPL_PANEL_SLICES)          (0: from the mean phase)
 *   SPL_PANEL_FORM_RING_K1     ring form on the paired storage: a few wavefronts of      units in flight per loader
 *   ..._K2, _K3, _K4, _K8      the workgroup only stream the image and hand it to the    (0: 6)
 *                              others, which only gather and fold, through 1.5 KiB
 *                              slots in LDS; 1 / 2 / 3 / 4 / 8 index blocks per phase;
 *                              rows_per_panel has to leave room for the slots (19 700
 *                              with the default 4 loaders)
 *   SPL_PANEL_FORM_ROUNDS      rounds form on the paired storage: fixed rounds of        pairs per wavefront and register
 *                              16 * unroll pairs whatever the index blocks are; no       set: 3 ... 6 (0: 5); anything
 *                              column slices                                             else is refused here
 * A chunk or paired request between the instantiated counts is served by the nearest kernel; a ring shape
 * (SPL_PANEL_RING_NL / _SLOTS / _GD with the form's blocks per phase and unroll) that is not instantiated is
 * refused by the first spl_matrix_spmv_dev with SPL_ERROR_argument_missing.  Any other form code is refused here.
 * Used by variant 16, and by variant 0 once spl_matrix_set_spmv_order(H, SPL_ORDER_FREE) was called. */
#define SPL_PANEL_FORM_DEFAULT 0
#define SPL_PANEL_FORM_CHUNK_K1 1
#define SPL_PANEL_FORM_CHUNK_K2 2
#define SPL_PANEL_FORM_PAIRED_K1 4
#define SPL_PANEL_FORM_PAIRED_K2 5
#define SPL_PANEL_FORM_RING_K1 6
#define SPL_PANEL_FORM_RING_K2 7
#define SPL_PANEL_FORM_RING_K3 8
#define SPL_PANEL_FORM_RING_K4 9
#define SPL_PANEL_FORM_RING_K8 10
#define SPL_PANEL_FORM_ROUNDS 11
int spl_matrix_build_panel(void *H, int rows_per_panel, int cols_log2, int unroll, int form);
/* Diagnostics: synchronises the device and returns 1 when a bounded wait of the ring form's hand-over gave
 * up during the last panel SpMV of this handle (its result is then invalid), 0 otherwise, < 0 on error. */
int spl_matrix_panel_errors(void *H);
/* the kernel spl_matrix_spmv_dev launches for this handle now: 0 CSR-stream, 8 column-blocked
 * lockstep, 15 sliced ELL, 16 column-sorted panels (other values: the forced ablation variant) */
int spl_matrix_spmv_kernel(void *H);

/* ---- one-sided exchange of y for the row-partitioned SpMV (one process per GPU; csrc/peer.hip) ----
 * Every rank pushes its block of y straight into every peer's copy with device-to-device copies on one
 * stream per peer (no collective kernel, no CU taken from the SpMV), then a 4-byte step flag; a one-thread
 * kernel on the compute stream waits for the N - 1 flags.  Peers' buffers are reached through IPC memory
 * handles that the caller passes between the processes (3 x 64 bytes per rank).
 * create: y is cut into chunks * world pieces, piece q = c * world + p = y[bounds[q], bounds[q+1]) belongs to
 *   rank p (chunks = 1: one block per rank); handles_out = this rank's 192 bytes.
 * connect: all_handles = world x 192 bytes in rank order.
 * A step = one push per chunk + finish.  push: the rank's piece of chunk c (produced on `stream`) goes to every
 *   rank (the copies run on the per-peer streams, i.e. under whatever `stream` does next — the kernel of the
 *   next chunk).  finish: after the work enqueued here *y_full (n doubles, device, valid until the step after
 *   next) is the whole y.  No host synchronisation.
 * failed: 1 if a wait gave up after ~2 s (a peer did not deliver). */
int spl_peer_exchange_create(int rank, int world, int chunks, int64_t n, const int64_t *bounds,
                             unsigned char *handles_out, void **X);
int spl_peer_exchange_connect(void *X, const unsigned char *all_handles);
int spl_peer_exchange_push(void *X, int chunk, const double *d_piece, void *stream);
int spl_peer_exchange_finish(void *X, void *stream, double **y_full);
int spl_peer_exchange_failed(void *X);
/* 1 when the step flags live in fine-grained device memory (polled by a kernel while a peer's copy engine
 * writes them: csrc/peer.hip), 0 when the runtime refused it and plain device memory is used */
int spl_peer_exchange_flags_finegrained(void *X);
void spl_peer_exchange_free(void **X);

/* fill a device vector with the synthetic entries j in [j0,j1) */
int spl_vector_synthetic_dev(uint64_t seed, int64_t j0, int64_t j1, double *d_x, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_LINEAR_HIP_H */

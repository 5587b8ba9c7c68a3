// common.hpp — shared host-side plumbing of the gfx950 backend.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <memory>
#include <new>
#include <vector>

#include "../../include/sparse_linear_hip.h"

namespace spl {

// thread-local text of the last HIP failure, returned by spl_last_error()
void set_last_error(const char *where, hipError_t e);
void set_last_error_text(const char *text);

struct DeviceError {
  int status;
};

#define SPL_HIP(expr)                                                        \
  do {                                                                       \
    hipError_t e_ = (expr);                                                  \
    if (e_ != hipSuccess) {                                                  \
      ::spl::set_last_error(#expr, e_);                                      \
      throw ::spl::DeviceError{e_ == hipErrorOutOfMemory ? SPL_ERROR_out_of_memory \
                                                         : SPL_ERROR_device}; \
    }                                                                        \
  } while (0)

// device memory for DBuf (device_pool.hip): large blocks are kept on release and reused
void *device_alloc(size_t bytes);
void device_free(void *p) noexcept;
size_t device_free_bytes();      // free memory as the driver reports it + what the pool would give back
size_t device_release_cached();  // returns the bytes given back to the driver
double device_alloc_seconds();  // seconds spent inside hipMalloc so far (pool misses)
// Non-blocking streams, kept for the life of the process (device_pool.hip): creating one costs 0.3 - 0.6 ms here and the
// first of a process 15 ms; the analysis takes four for its level structures, a factorisation seventeen per host thread.
hipStream_t pooled_stream_take(int device);            // an idle one of this device, or a new one (nullptr: creation failed)
void pooled_stream_give(int device, hipStream_t s);    // back, once its work is complete
void pooled_streams_prewarm(int device, int count);    // create streams until `count` are idle (another thread may take them meanwhile)

// RAII device buffer, movable
template <typename T>
struct DBuf {
  T *p = nullptr;
  size_t n = 0;
  DBuf() = default;
  explicit DBuf(size_t count) { alloc(count); }
  DBuf(const DBuf &) = delete;
  DBuf &operator=(const DBuf &) = delete;
  DBuf(DBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DBuf &operator=(DBuf &&o) noexcept {
    if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
    return *this;
  }
  ~DBuf() { release(); }
  void alloc(size_t count) {
    release();
    n = count;
    // +64 B slack: vector loads of the streaming kernels may read (never use) a
    // few elements past the logical end
    p = static_cast<T *>(device_alloc((count ? count : 1) * sizeof(T) + 64));
  }
  void release() {
    if (p) { device_free(p); p = nullptr; n = 0; }
  }
  T *get() const { return p; }
};

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Kernel attributes (hipFuncSetAttribute: dynamic LDS above 64 KB) are per DEVICE: a `static bool` would leave the second
// GPU of a process without them.  One bit per device in a mask per call site; true for the first caller on the current
// device.  (Two threads racing on the first use both set the attributes: the loser of fetch_or still proceeds only
// after its own check below, and setting them twice is harmless.)
inline bool first_use_on_this_device(std::atomic<uint64_t> &mask) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return true;
  const uint64_t bit = 1ull << (dev & 63);
  return (mask.load(std::memory_order_acquire) & bit) == 0;
}
inline void mark_used_on_this_device(std::atomic<uint64_t> &mask) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  mask.fetch_or(1ull << (dev & 63), std::memory_order_release);
}

// sets the device for the current thread and restores the previous one on exit
struct DeviceGuard {
  int prev = -1;
  bool changed = false;
  explicit DeviceGuard(int dev) {
    SPL_HIP(hipGetDevice(&prev));
    if (prev != dev) { SPL_HIP(hipSetDevice(dev)); changed = true; }
  }
  ~DeviceGuard() {
    if (changed) (void)hipSetDevice(prev);
  }
};

constexpr uint32_t kMatrixMagic = 0x53504C4Du;  // "SPLM"

// What every other object behind a handle begins with (it is the object's first base): the C boundary (abi.hip) tells
// the objects apart by the magic word and compares devices, sizes and value kinds without seeing their types.
struct ObjectHead {
  uint32_t magic;
  int device = 0;
  int vw = 1;     // doubles per entry: 1 real, 2 packed complex
  int64_t n = 0;  // rows
  explicit ObjectHead(uint32_t word) : magic(word) {}
};
constexpr uint32_t kTriMagic = 0x53504C54u;     // "SPLT"
constexpr uint32_t kIluMagic = 0x53504C49u;     // "SPLI"
constexpr uint32_t kKrylovMagic = 0x53504C4Bu;  // "SPLK"
constexpr uint32_t kAmgMagic = 0x53504C47u;     // "SPLG"
constexpr uint32_t kGmresMagic = 0x53504C47u;   // "SPLG": the word of the AMG object, so the two are not told apart
constexpr uint32_t kEigshMagic = 0x53504C45u;   // "SPLE"
constexpr uint32_t kLobpcgMagic = 0x53504C42u;  // "SPLB": the block eigensolver
// the object behind h, or nullptr unless h carries the magic word
template <typename T, uint32_t Magic>
T *as_object(void *h) {
  const ObjectHead *o = static_cast<const ObjectHead *>(h);
  return (o && o->magic == Magic) ? static_cast<T *>(h) : nullptr;
}
// the head of an object whose type the caller does not see (the head lies at the object's address)
template <typename T>
const ObjectHead &head(const T *object) { return *reinterpret_cast<const ObjectHead *>(object); }
// the end of an object: the handle stops being one before the memory goes
template <typename T>
void delete_object(T *object) {
  object->magic = 0;
  delete object;
}

// column-blocked image of a row block (spmv_blocked.hip)
struct BlockedImage {
  int R = 0, w = 0;               // panel = R rows (R << w must fit 31 bits), column block = 2^w columns
  int64_t npanels = 0, ncb = 0;
  DBuf<int64_t> segptr;           // npanels*ncb + 1
  DBuf<int> key;                  // nnz: (local_row << w) | local_col
  DBuf<double> val;               // nnz
  DBuf<unsigned> arrive;          // rendezvous counter of the persistent kernel
  int fold = 1;                   // 1: ds_add_f64 fold, 0: shuffle fold (both reference order)
  int lockstep_waves = 16;        // wavefronts (= panels) per lockstep workgroup: 16 or 8; 0 = ablation kernel
};

// What one launch of the panel SpMV runs (spmv_panel.hip): the form and its numbers.  Made from the ABI's form code
// by panel_plan_from_code / choose_panel_plan; the kernels that exist are the table in spmv_panel.hip.
enum class PanelForm {
  Chunk,   // one chunk per load, phases of kblocks index blocks
  Paired,  // paired storage (a pair of chunks per 8-byte key / 16-byte value load), phases, optional column slices
  Rounds,  // paired storage, fixed rounds of 16 * sets units whatever the index blocks are
  Ring     // paired storage, loader wavefronts hand units to gather wavefronts through LDS slots
};
struct PanelPlan {
  PanelForm form = PanelForm::Chunk;
  int sets = 0;                   // register sets per wavefront (chunks, or pairs of them); ring: units in flight per loader
  int kblocks = 2;                // index blocks per phase (barrier to barrier); not used by the rounds form
  int nslices = 1;                // paired form: column slices per panel (8 = one per XCD)
  int ablate = 0;                 // chunk form: timing-only ablation bits (SPL_PANEL_ABLATE with SPL_ALLOW_ABLATION=1)
  int nl = 4, gather = 4, slots = 1;  // ring form: loaders, units in flight per gatherer, slots per loader
  int meet = 1;                   // rounds form: 1 = all workgroups meet between their panels (the rendezvous), 0 = each goes on at once
};

// workgroup-wide column-sorted panels of a row block (spmv_panel.hip): the order-free SpMV mode
struct PanelImage {
  int P = 0, w = 0;               // panel = P rows (one workgroup's LDS), index block = 2^w columns (w <= 17)
  int64_t npanels = 0, nib = 0, nchunks = 0;
  DBuf<int> segc;                 // npanels*nib + 1 (+ padding): first 64-entry chunk of each segment
  DBuf<unsigned> key;             // (local_col << 15) | local_row, segments padded to whole chunks
  DBuf<double> val;
  DBuf<int> ublk;                 // paired storage: index block of every unit (pair of chunks), for the rounds form
  DBuf<unsigned> arrive;          // the sync words: rendezvous between generations, ring form's error word, rounds form's leave count
  int pair = 0;                   // 1: paired storage (chunk pairs interleaved, 8-byte key / 16-byte value loads)
  PanelPlan plan;                 // what spl_matrix_spmv_dev launches on this image
};

// sliced-ELL image of a row block (spmv_sell.hip)
struct SellImage {
  int64_t nslices = 0, entries = 0;
  DBuf<int64_t> sliceoff;  // nslices + 1, in units of 64 entries
  DBuf<int> col;
  DBuf<double> val;
};

// A device-resident block of rows [row0, row0+nrows_local) of a sparse matrix
// with nrows_global x ncols entries, stored row-major (CSR, int32 column
// indices, int64 row pointers relative to the block).
struct Matrix {
  uint32_t magic = kMatrixMagic;
  int device = 0;
  int64_t nrows_global = 0, ncols = 0, row0 = 0, nrows_local = 0, nnz = 0;
  DBuf<int64_t> rowptr64;  // nrows_local+1, always present
  DBuf<int> rowptr;        // nrows_local+1, present iff nnz < 2^31
  DBuf<int> colidx;        // nnz
  DBuf<double> val;        // nnz
  int vw = 1;              // doubles per stored value: 1 Double, 2 packed Complex Double (csrc/spmv_z.hip)
  int variant = 0;
  int64_t max_row_len = 0;
  double new_line_fraction = -1.0;  // share of entries whose x line the previous row did not touch; < 0: not measured yet
  BlockedImage *blocked = nullptr;  // built on demand (spl_matrix_build_blocked / auto)
  SellImage *sell = nullptr;        // built on demand (spl_matrix_optimize on regular matrices)
  PanelImage *panel = nullptr;      // built on demand (spl_matrix_build_panel / spl_matrix_set_spmv_order)
  int blocked_unroll = 0;  // 0 = default; < 0 selects the ablation kernel
  int reserved_cus = -1;    // spl_matrix_set_reserved_cus: CUs left to a communication kernel; < 0: SPL_SPMV_RESERVED_CUS or 0
  bool order_free = false;  // spl_matrix_set_spmv_order: variant 0 may use the panel image (1e-10, order-free sums)
  Matrix() = default;
  Matrix(const Matrix &) = delete;
  Matrix &operator=(const Matrix &) = delete;
  ~Matrix() { delete blocked; delete sell; delete panel; }
};

inline Matrix *as_matrix(void *h) {
  Matrix *m = static_cast<Matrix *>(h);
  return (m && m->magic == kMatrixMagic) ? m : nullptr;
}

// ---- device primitives (scan.hip) -------------------------------------------------
// exclusive prefix sum of n counts; out has n+1 entries (out[n] = total).
void exclusive_scan_i32_to_i64(const int *d_in, int64_t *d_out, int64_t n, hipStream_t s);
void exclusive_scan_i64(const int64_t *d_in, int64_t *d_out, int64_t n, hipStream_t s);
// radix_sort.hip: LSD radix sort of 64-bit keys by their bits [0, nbits); returns the buffer holding the result
size_t radix_sort_u64_temp_bytes(int64_t n);
unsigned long long *radix_sort_u64(unsigned long long *keys, unsigned long long *alt, int64_t n, int nbits, void *temp,
                                   hipStream_t s);
void narrow_i64_to_i32(const int64_t *d_in, int *d_out, int64_t n, hipStream_t s);
void widen_i32_to_i64(const int *d_in, int64_t *d_out, int64_t n, hipStream_t s);

// ---- CSR image construction (convert.hip) ------------------------------------------
// validate a CSC/CSR pointer+index pair on the device: ptr[0]==0, monotone,
// ptr[nmajor]==nnz, 0 <= idx < nminor.  Returns SPL_OK or SPL_ERROR_invalid_matrix.
int validate_compressed(const int *d_ptr, const int *d_idx, int64_t nmajor, int64_t nminor,
                        int64_t nnz, hipStream_t s);
// Order-preserving transpose of compressed arrays (nmajor slices over nminor
// indices): out_ptr64[nminor+1], out_idx[nnz], out_val[nnz]; inside each new
// slice the old major index ascends (Sparse.hs:301-329).
void transpose_compressed(const int *d_ptr, const int *d_idx, const double *d_val, int64_t nmajor,
                          int64_t nminor, int64_t nnz, int64_t *out_ptr64, int *out_idx,
                          double *out_val, hipStream_t s);
// sort every segment [ptr[i], ptr[i+1]) of (key, val) pairs by key ascending
void segmented_sort_pairs(const int64_t *d_ptr64, int64_t nseg, int *d_key, double *d_val,
                          hipStream_t s);
// same, but segments longer than max_len are left untouched (already sorted)
void segmented_sort_pairs_capped(const int64_t *d_ptr64, int64_t nseg, int *d_key, double *d_val,
                                 int64_t max_len, hipStream_t s);
void segmented_sort_pairs64(const int64_t *d_ptr64, int64_t nseg, int64_t *d_key, double *d_val,
                            hipStream_t s);
void segmented_sort_pairs_u32(const int64_t *d_ptr64, int64_t nseg, unsigned *d_key, double *d_val,
                              hipStream_t s);
// finish a Matrix whose rowptr64/colidx/val are filled: int32 pointers, stats
void finalize_matrix(Matrix *m, hipStream_t s);
// CUs of a device, asked once per device, not per launch; 0 when the runtime refuses
inline int device_cus(int device) {
  static std::atomic<int> cus_of[64];
  int cus = cus_of[device & 63].load(std::memory_order_relaxed);
  if (cus == 0 && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess)
    cus_of[device & 63].store(cus, std::memory_order_relaxed);
  return cus;
}
int spmv_cus(const Matrix *m);  // CUs the persistent SpMV images are laid out for: the device's minus the reserved ones
void measure_locality(Matrix *m, hipStream_t s);  // fills new_line_fraction on first call

// ---- assembly (assemble.hip) ------------------------------------------------------------
int compress_device(int nrows, int ncols, int64_t nnz, const int *d_rows, const int *d_cols,
                    const double *d_vals, int *d_newptr, DBuf<int> &out_idx, DBuf<double> &out_val,
                    int64_t *nnz_out, int64_t *bad, hipStream_t s, bool check_only = false);
// the same for indices of index_width 4 or 8 bytes, compared with the bounds in that width, and values of vw doubles
int compress_device_wide(int index_width, int vw, int64_t nrows, int64_t ncols, int64_t nnz, const void *d_rows,
                         const void *d_cols, const double *d_vals, int *d_newptr, DBuf<int> &out_idx,
                         DBuf<double> &out_val, int64_t *nnz_out, int64_t *bad, hipStream_t s, bool check_only = false);
bool columns_sorted(const int *d_ptr, const int *d_idx, int64_t ncols, hipStream_t s);
void lin_device(double alpha, const int *Ap, const int *Ai, const double *Ax, double beta, const int *Bp,
                const int *Bi, const double *Bx, int64_t ncols, DBuf<int64_t> &Cp, DBuf<int> &Ci,
                DBuf<double> &Cx, int64_t *nnzC, hipStream_t s);
void lin_device_z(const double alpha[2], const int *Ap, const int *Ai, const double *Az, const double beta[2],
                  const int *Bp, const int *Bi, const double *Bz, int64_t ncols, DBuf<int64_t> &Cp, DBuf<int> &Ci,
                  DBuf<double> &Cz, int64_t *nnzC, hipStream_t s);

// ---- compressed arrays in device memory, in and out (device_arrays.hip) --------------------------------------------
// index_width: bytes per element of the caller's pointer and index arrays, 4 or 8; every comparison is made in that width
// Pointers: [0] == 0, none negative, none above its successor; copied to out_ptr64[nmajor + 1] in the same pass.
// Returns nnz = ptr[nmajor], or -1 for an invalid array (one 8-byte read-back; synchronises s).
int64_t import_pointers(int index_width, const void *d_ptr, int64_t nmajor, int64_t *out_ptr64, hipStream_t s);
// Indices: each in [0, nminor), narrowed to out_idx[nnz] in the same pass.  SPL_OK or SPL_ERROR_invalid_matrix.
// ascending != nullptr: also *ascending = every slice of d_ptr64 ascends strictly.  Synchronises s.
int import_indices(int index_width, const void *d_idx, int64_t nnz, int64_t nminor, const int64_t *d_ptr64,
                   int64_t nmajor, int *out_idx, bool *ascending, hipStream_t s);
// false when the runtime knows the allocation d_p lies in and fewer than `bytes` bytes of it follow d_p: a pointer array
// whose last entry promises more entries than the caller's arrays can hold is refused before anything is read
bool device_range_holds(const void *d_p, size_t bytes);

// ---- the structural constructors on handles (assemble_handles.hip) -----------------------------------------
// C's dimensions, block and value kind are set by the caller; these fill rowptr64 / colidx / val / nnz on stream s
void kronecker_handles(const Matrix *A, const Matrix *B, Matrix *C, hipStream_t s);
// host: the interval table of nblocks placed rectangles; SPL_ERROR_dimension_mismatch when one leaves the
// nrowsC x ncolsC result or two overlap
int blocks_table(int nblocks, const Matrix *const *blk, const int64_t *row_off, const int64_t *col_off, int64_t nrowsC,
                 int64_t ncolsC, std::vector<int> &cut, std::vector<int> &lptr, std::vector<int> &list);
void assemble_handles(int nblocks, const Matrix *const *blk, const int64_t *row_off, const int64_t *col_off,
                      const std::vector<int> &cut, const std::vector<int> &lptr, const std::vector<int> &list, Matrix *C,
                      hipStream_t s);
void take_diag_handle(const Matrix *A, int64_t n, double *d, hipStream_t s);  // enqueues; does not synchronise
void diag_handle(const double *d_values, Matrix *C, hipStream_t s);           // d_values == nullptr: ones

// ---- windows and selections of handles (submatrix.hip) -------------------------------------------------------
// C's dimensions and value kind are set by the caller, A is whole and the arguments are checked; both synchronise s
void submatrix_handle(const Matrix *A, int64_t r0, int64_t c0, Matrix *C, hipStream_t s);
// C[i, j] = A[I[i], J[j]], source order kept inside the rows; *ascending == false: the caller sorts them.  nullptr for
// d_I / d_J: all rows / columns.  SPL_ERROR_index_out_of_bounds (*bad: first offending position, I before J) or
// SPL_ERROR_invalid_matrix (a column named twice)
int select_handle(const Matrix *A, int index_width, const void *d_I, const void *d_J, Matrix *C, bool *ascending,
                  int64_t *bad, hipStream_t s);

// ---- entry-wise maps, scaling, filters and reductions on handles (entrywise.hip) -----------------------------
// C's dimensions, block and value kind are set by the caller and the arguments are checked; the four that make a
// handle fill rowptr64 / colidx / val / nnz and synchronise s.  A may be a row block.
void map_handle(const Matrix *A, int op, double sre, double sim, Matrix *C, hipStream_t s);
void scale_rows_cols_handle(const Matrix *A, const double *d_r, const double *d_c, Matrix *C, hipStream_t s);
void filter_handle(const Matrix *A, int keep, double tol, Matrix *C, hipStream_t s);
void band_handle(const Matrix *A, int64_t lo, int64_t hi, Matrix *C, hipStream_t s);  // lo > hi: `zeros`
// enqueues on s; the column sums (axis 0, abs_sum) hold temporaries and synchronise s
void reduce_handle(const Matrix *A, int what, int axis, double *d_out, hipStream_t s);
double norm_handle(const Matrix *A, int which, hipStream_t s);  // synchronises s

// ---- sparse triangular solves on handles (trisolve.hip, tri_levels.hpp) ----------------------------------------
struct TriSolver;
inline TriSolver *as_trisolver(void *t) { return as_object<TriSolver, kTriMagic>(t); }
// A: whole, square, 32-bit row pointers (the caller checked).  SPL_OK or SPL_WARNING_singular_matrix; synchronises
int trisolve_analyze(const Matrix *A, int uplo, int diag, TriSolver **out);
// enqueues on s; the first solve with a transposed op builds that image under the object's lock and synchronises
int trisolve_solve(TriSolver *T, int op, int k, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, hipStream_t s);
void trisolve_info(const TriSolver *T, int64_t info[8]);
void trisolve_delete(TriSolver *T);

// ---- ILU(0) on handles (ilu0.hip, tri_levels.hpp): the producer of what the triangular solves apply -------------
struct IluPlan;
inline IluPlan *as_ilu_plan(void *p) { return as_object<IluPlan, kIluMagic>(p); }
// A: whole, square, 32-bit row pointers (the caller checked).  SPL_OK; synchronises
int ilu0_analyze(const Matrix *A, IluPlan **out);
// A: whole, 32-bit row pointers, on the plan's device (the caller checked); C: dimensions and value kind set by the
// caller.  SPL_ERROR_invalid_matrix (A's pattern is not the analysed one; C stays empty), else C holds A's pattern and
// the L\U values (rowptr64 / colidx / val / nnz): SPL_OK or SPL_WARNING_singular_matrix.  Synchronises s
int ilu0_factor(IluPlan *P, const Matrix *A, Matrix *C, hipStream_t s);
void ilu0_info(const IluPlan *P, int64_t info[8]);
void ilu0_delete(IluPlan *P);

// ---- the fixed-order inner product, preconditioned CG and BiCGSTAB on handles (krylov.hip) ----------------------
// <a,b> of n entries of vw doubles each to d_out (vw doubles, device memory); enqueues on s, no synchronisation
int vector_dot(int device, int64_t n, int vw, const double *d_a, const double *d_b, double *d_out, hipStream_t s);
struct Krylov;
inline Krylov *as_krylov(void *k) { return as_object<Krylov, kKrylovMagic>(k); }
// A: whole and square (the caller checked); borrowed.  SPL_OK
int krylov_create(const Matrix *A, int method, Krylov **out);
// the parts are borrowed and of K's size and value kind (the caller checked); nullptr: the part is the identity
void krylov_set_preconditioner(Krylov *K, TriSolver *T1, const double *d_mid, TriSolver *T2);
// n > 0 and the arguments are checked by the caller; enqueues on s and synchronises it (the outcome is read back)
int krylov_solve(Krylov *K, const double *d_b, double *d_x, int use_x0, double rtol, double atol, int64_t max_iter,
                 int check_every, int64_t result[4], double *history, hipStream_t s);
void krylov_info(Krylov *K, int64_t info[8]);
void krylov_delete(Krylov *K);

// ---- multicolour ordering on handles (coloring.hip) -----------------------------------------------------------------
// A: whole, square, 32-bit row pointers (the caller checked).  d_colors: n ints; d_perm: n ints or nullptr; offsets:
// nullptr, or where a malloc()'d array of info[1] + 1 class boundaries goes.  Default stream; synchronises.  SPL_OK
int color_handle(const Matrix *A, uint64_t seed, int *d_colors, int *d_perm, int64_t **offsets, int64_t info[8]);
// out[k] = in[perm[k]] (inverse == 0) or out[perm[k]] = in[k], entries of vw doubles moved as bits; n > 0; enqueues on s
void vector_permute(int64_t n, int vw, const int *d_perm, int inverse, const double *d_in, double *d_out, hipStream_t s);
// The priority both the colouring and the aggregation order the vertices by: the splitmix64 finaliser of v + base,
// base = kColorGolden * (seed + 1); u precedes v when h(u) > h(v), or they are equal and u < v
constexpr uint64_t kColorGolden = 0x9E3779B97F4A7C15ull;
__host__ __device__ inline uint64_t color_priority(uint64_t v, uint64_t base) {
  uint64_t z = v + base;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// The graph both the colouring and the aggregation walk: A's pattern and the pattern of its transpose (rows unordered);
// {i, j}, i != j, is an edge when it is stored on either side
struct ColorGraph {
  const int *ptr;       // n + 1
  const int *col;       // nnz
  const int64_t *tptr;  // n + 1
  const int *tcol;      // nnz
};
struct ColorGraphBuffers {
  DBuf<int> counts, tcol;
  DBuf<int64_t> tptr;
};
// A: whole, square, 32-bit row pointers, n > 0.  The transposed pattern goes to buf; *launches grows by the kernels
ColorGraph build_color_graph(const Matrix *A, int64_t grid_cap, ColorGraphBuffers &buf, int64_t *launches, hipStream_t s);
// *d_max_degree (zeroed by the caller): the largest number of distinct neighbours; G lanes a vertex; one launch on s
void color_graph_max_degree(const ColorGraph &graph, int n, int G, int64_t grid_cap, int *d_max_degree, hipStream_t s);

// ---- aggregation AMG on handles (amg.hip) ---------------------------------------------------------------------------
// A: whole, square, 32-bit row pointers (the caller checked).  d_agg: n ints; d_roots: n ints or nullptr.  Default
// stream; synchronises.  SPL_OK
int aggregate_handle(const Matrix *A, uint64_t seed, int *d_agg, int *d_roots, int64_t info[8]);
struct Amg;
inline Amg *as_amg(void *m) { return as_object<Amg, kAmgMagic>(m); }
// A: whole and square (the caller checked), borrowed; opt: the eight options with the defaults filled in and checked
int amg_create(Matrix *A, const int64_t opt[8], Amg **out);
void amg_info(Amg *M, int64_t info[8]);
// level in [0, levels): the level's handles (P and R nullptr on the coarsest), its weights and {n_l, n_{l+1} or 0}
void amg_level(Amg *M, int level, void **HA, void **HP, void **HR, const double **d_w, int64_t dims[2]);
// x = cycle(0, b); d_b != d_x (the caller checked); enqueues on s.  *launches (may be nullptr): kernels enqueued
int amg_apply(Amg *M, const double *d_b, double *d_x, hipStream_t s, int64_t *launches);
void amg_delete(Amg *M);
// M: borrowed, of K's size, value kind and device (the caller checked), or nullptr; clears the triangular parts
void krylov_set_preconditioner_amg(Krylov *K, Amg *M);

// ---- a block of inner products in one pass (gram.hip) --------------------------------------------------------------------
// G[i][j] = <V[:, i], W[:, j]>, i < k, j < l, of n entries of vw doubles each to d_G (column major, entry (i, j) at
// d_G + (j * ldg + i) * vw; upper: only i <= j is written).  Each value is vector_dot's, bit for bit; enqueues on s;
// *launches (may be nullptr) grows by the kernels enqueued, whatever the cut into blocks of columns is
int vector_gram(int device, int64_t n, int vw, int k, int l, const double *d_V, int64_t ldv, const double *d_W,
                int64_t ldw, double *d_G, int64_t ldg, int upper, hipStream_t s, int64_t *launches = nullptr);

// ---- restarted GMRES on handles and the fused multi-vector inner product (gmres.hip) ---------------------------------
// <V[:, i], w>, i < k, of n entries of vw doubles each to d_out (k entries, device memory); column i starts at
// d_V + i * ldv * vw.  Each value is vector_dot's, bit for bit; enqueues on s, no synchronisation
int vector_dots(int device, int64_t n, int vw, int k, const double *d_V, int64_t ldv, const double *d_w, double *d_out,
                hipStream_t s);
struct Gmres;
inline Gmres *as_gmres(void *g) { return as_object<Gmres, kGmresMagic>(g); }
// A: whole and square, 1 <= restart <= 128 (the caller checked); borrowed.  SPL_OK
int gmres_create(const Matrix *A, int restart, Gmres **out);
// the parts are borrowed and of G's size, value kind and device (the caller checked); nullptr: the identity
void gmres_set_preconditioner(Gmres *G, TriSolver *T1, const double *d_mid, TriSolver *T2);
void gmres_set_preconditioner_amg(Gmres *G, Amg *M);
// n > 0 and the arguments are checked by the caller; enqueues on s and synchronises it (the outcome is read back)
int gmres_solve(Gmres *G, const double *d_b, double *d_x, int use_x0, double rtol, double atol, int64_t max_iter,
                int check_every, int64_t result[6], double *history, double residual[2], hipStream_t s);
void gmres_info(Gmres *G, int64_t info[8]);
void gmres_delete(Gmres *G);

// ---- thick-restart Lanczos on handles and the in-place basis rotation (eigsh.hip) ---------------------------------------
// V[:, :k] <- V Y (d_out == nullptr) or d_out = V Y: V n x m entries of vw doubles, Y real m x k, all column major in
// device memory; 1 <= k <= m <= 128 and d_out clear of V (the caller checked); enqueues on s, no synchronisation
// y_complex (vw == 2 only): Y holds packed pairs and a term is Data.Complex's product (spl_vector_rotate_z_dev)
int vector_rotate(int64_t n, int vw, int m, int k, double *d_V, int64_t ldv, const double *d_Y, int ldy, double *d_out,
                  int64_t ldo, hipStream_t s, bool y_complex = false);
struct Eigsh;
inline Eigsh *as_eigsh(void *e) { return as_object<Eigsh, kEigshMagic>(e); }
// A: whole, square and Hermitian, 2 <= ncv <= 128 (the caller checked); borrowed.  SPL_OK
int eigsh_create(const Matrix *A, int ncv, Eigsh **out);
// K: borrowed, of E's size, value kind and device (the caller checked), or nullptr: the operator is A again
void eigsh_set_inverse(Eigsh *E, Krylov *K, double sigma, double rtol, double atol, int64_t max_iter);
// n > 0 and the arguments are checked by the caller; enqueues on s and synchronises it (the outcome is read back)
int eigsh_solve(Eigsh *E, int nev, int which, double tol, double atol, int64_t max_restarts, const double *d_v0,
                double *values, double *d_vectors, int64_t ldx, double *residuals, int64_t result[6], double *history,
                hipStream_t s);
void eigsh_info(Eigsh *E, int64_t info[8]);
int eigsh_ncv(const Eigsh *E);
void eigsh_delete(Eigsh *E);

// ---- LOBPCG on handles (lobpcg.hip) ---------------------------------------------------------------------------------------
struct Lobpcg;
inline Lobpcg *as_lobpcg(void *l) { return as_object<Lobpcg, kLobpcgMagic>(l); }
// A: whole, square and Hermitian, 1 <= block <= 42 (the caller checked); borrowed.  SPL_OK
int lobpcg_create(const Matrix *A, int block, Lobpcg **out);
// the parts are borrowed and of L's size, value kind and device (the caller checked); nullptr: the identity
void lobpcg_set_preconditioner(Lobpcg *L, TriSolver *T1, const double *d_mid, TriSolver *T2);
void lobpcg_set_preconditioner_amg(Lobpcg *L, Amg *M);
// n > 0 and the arguments are checked by the caller; enqueues on s and synchronises it (the outcome is read back)
int lobpcg_solve(Lobpcg *L, int nev, int which, double tol, double atol, int64_t max_iter, const double *d_X0,
                 int64_t ldx0, double *values, double *d_vectors, int64_t ldx, double *residuals, int64_t result[8],
                 double *history, hipStream_t s);
void lobpcg_info(Lobpcg *L, int64_t info[8]);
// B: borrowed; whole, square, Hermitian and of L's size, value kind and device (the caller checked), or nullptr: the
// standard problem again, and the vectors of B S are released
void lobpcg_set_mass(Lobpcg *L, const Matrix *B);
// w = ((w - c_0 v_0) - ...) and bw = ((bw - c_0 (Bv)_0) - ...) over k columns in one pass, and Re<w, bw> of the results
// to d_q (may be nullptr), the real part of vector_dot's value bit for bit; enqueues on s, no synchronisation
int vector_update_pair(int device, int64_t n, int vw, int k, const double *d_V, int64_t ldv, const double *d_BV,
                       int64_t ldbv, const double *d_coef, double *d_w, double *d_bw, double *d_q, hipStream_t s);
int lobpcg_block(const Lobpcg *L);
void lobpcg_delete(Lobpcg *L);

// ---- multifrontal LU without interchanges (multifrontal.hip, mf_symbolic.hpp) ------------------
namespace mf {
struct Tree;
struct Factors;
struct LevelService;
}  // namespace mf
// level structures of the nested dissection's large regions on the GPU (nd_levels.hip); nullptr: no usable device
std::unique_ptr<mf::LevelService> make_gpu_level_service(int n, int64_t max_adj);
size_t mf_device_bytes(const mf::Tree &T, int zm = 1);  // zm = 2: complex fronts (two planes)
mf::Factors *mf_factor(std::shared_ptr<const mf::Tree> tree, const int *d_Ap, const int *d_Ai, const double *d_Ax,
                       const int *d_Rp, const int *d_Rj, const double *d_Rx, const int *d_perm, const int *d_inv,
                       hipStream_t s, bool symmetric = false, bool zfront = false, bool pivot = false,
                       const double *d_rscale = nullptr);  // pivot: threshold pivoting inside the diagonal blocks, on
                                                           // candidates scaled by d_rscale (new ordering of `tree`)
int mf_singular(const mf::Factors *F);
// the chain matrices of the large fronts' pivot blocks (mf_chain.hpp): out[0] bytes of device memory, out[1] milliseconds
// their construction took, out[2] pivots per block (0: no chains)
void mf_chain_info(const mf::Factors *F, double out[3]);
void mf_solve(const mf::Factors *F, int sys, double *d_c, int k, size_t stride, hipStream_t s);
void mf_free(mf::Factors *F);
// where the pivots of multifrontal factors lie (determinant.hip reads them): pivot g (new ordering) of real fronts is
// arena[poff[f] + j (ldp[f] + 1)], f = front_of[g], j = g - p0[f]; the inverse of diagonal block b of front f (threshold
// pivoting: inv(L11) P_b) is at invs + ioff[f] + b 2 64 64.  Device pointers except the host tree.
struct MfPivots {
  const mf::Tree *tree;
  int zm;  // 2: complex fronts (not served)
  const double *arena, *invs;
  const int *front_of, *p0, *ldp;
  const int64_t *poff;
};
MfPivots mf_pivots(const mf::Factors *F);

// ---- SpGEMM (spgemm.hip) ------------------------------------------------------------------
void spgemm_device(int64_t nrowsA, int64_t ncolsA, const int *Ap, const int *Ai, const double *Ax,
                   int64_t ncolsB, const int *Bp, const int *Bi, const double *Bx, DBuf<int64_t> &Cp,
                   DBuf<int> &Ci, DBuf<double> &Cx, int64_t *nnzC, int64_t *products, hipStream_t s);

// mm on packed Complex Double (spgemm_z.hip): pattern from the real kernels, values in the reference's order
void spgemm_device_z(int64_t nrowsA, int64_t ncolsA, const int *Ap, const int *Ai, const double *Az, int64_t ncolsB,
                     const int *Bp, const int *Bi, const double *Bz, DBuf<int64_t> &Cp, DBuf<int> &Ci,
                     DBuf<double> &Cz, int64_t *nnzC, int64_t *products, hipStream_t s);

// ---- blocked band LU without interchanges (band_nopiv.hip) --------------------------------------
bool band_is_column_dominant(int n, const int *d_Ap, const int *d_Ai, const double *d_Ax, hipStream_t s);
// leading dimension of the band storage: >= kl+ku+1, padded so that the stride between the same row
// of adjacent columns (ldab-1 doubles) is an odd multiple of 128 bytes, not a power of two
inline int band_nopiv_ldab(int kl, int ku) {
  int l = kl + ku + 1;
  while ((l - 1) % 32 != 16) ++l;
  return l;
}
size_t band_nopiv_inverse_elems(int n);  // doubles needed for the per-block inverse factors
int band_nopiv_factor(int n, int kl, int ku, int ldab, double *d_AB, double *d_invs, const int *d_Ap, const int *d_Ai,
                      const double *d_Ax, const int *d_inv, hipStream_t s);
constexpr int kSolveGroup = 8;  // right-hand sides the blocked solves take through the band at once
void band_nopiv_solve(int sys, int n, int kl, int ku, int ldab, const double *d_AB, const double *d_invs, double *d_c,
                      int nrhs, size_t stride, hipStream_t s);

// ---- synthetic generators (generate.hip) --------------------------------------------
void generate_synthetic(Matrix *m, int kind, int64_t n_or_m, int K, uint64_t seed, hipStream_t s);
void generate_rmat_coo(uint64_t seed, int scale, uint32_t ta, uint32_t tb, uint32_t tc, int64_t nedges,
                       int *d_rows, int *d_cols, double *d_vals, hipStream_t s);
void generate_vector(uint64_t seed, int64_t j0, int64_t j1, double *d_x, hipStream_t s);

// ---- SpMV (spmv.hip) --------------------------------------------------------------------
// y = A x (accumulate == 0) or y <- A x + y, rows of the block; enqueued on s
int launch_spmv(const Matrix *m, const double *d_x, double *d_y, int accumulate, hipStream_t s);
// C (nrows_local x k, row-major) = A B (+ C) for a row-major dense B (ncols x k): one pass over A
int launch_spmm(const Matrix *m, const double *d_B, double *d_C, int k, int accumulate, hipStream_t s);
// Y[:, j] = A X[:, j] (+ Y[:, j]), j < k, on the CSR image of a real or complex handle (spmv_many.hip): X and Y
// column-major with leading dimensions ldx, ldy in entries (a double, or a packed pair); every (row, vector) sum in
// the reference's order whatever the row's length; SPL_OK at once for nrows_local == 0 or k == 0
int launch_spmv_many(const Matrix *m, int k, const double *d_X, int64_t ldx, double *d_Y, int64_t ldy, int accumulate,
                     hipStream_t s);
// d_out (cols x rows, row-major) = transpose of d_in (rows x cols, row-major); vw doubles per entry
int transpose_dense(int64_t rows, int64_t cols, int vw, const double *d_in, double *d_out, hipStream_t s);
// Complex Double (spmv_z.hip): d_x, d_y packed (re, im) pairs
int launch_spmv_z(const Matrix *m, const double *d_x, double *d_y, int accumulate, hipStream_t s);
void fill_positions(int64_t n, double *d_out, hipStream_t s);
// d_out[i] = d_in[d_pos[i]] on packed pairs; conjugate: (re, -im), the sign bit flipped (conj of Data.Complex)
void gather_complex_values(int64_t n, const double *d_pos, const double *d_in, double *d_out, hipStream_t s,
                           bool conjugate = false);
// `ctrans m == m` (Sparse.hs:377-379 under the derived Eq) on the CSR image of a whole square handle with strictly
// ascending indices, real or packed complex: 1 or 0, without building the transpose (hermitian.hip); synchronises s
int hermitian_device(const Matrix *m, hipStream_t s);
int64_t sell_padded_entries(const Matrix *m, hipStream_t s);
void build_sell_image(Matrix *m, hipStream_t s);
int launch_spmv_sell(const Matrix *m, const double *d_x, double *d_y, int accumulate, hipStream_t s);
constexpr int kNumSpmvVariants = 17;  // 16 = column-sorted workgroup panels (order-free);  // 15 = sliced-ELL image;  // 12-14: timing-only ablations of the CSR-stream kernel (wrong results)  // 0 auto, 1-6 CSR-stream shapes, 7 sub-wavefront, 8 column-blocked
void build_blocked_image(Matrix *m, int rows_per_panel, int w, hipStream_t s);
int launch_spmv_blocked(const Matrix *m, const double *d_x, double *d_y, int accumulate, int unroll,
                        hipStream_t s);
void build_panel_image(Matrix *m, int rows_per_panel, int w, int pair, hipStream_t s);
// runs `plan` (PanelImage::plan, or a candidate of the tuner) on m's panel image
int launch_spmv_panel(const Matrix *m, const PanelPlan &plan, const double *d_x, double *d_y, int accumulate, hipStream_t s);
size_t panel_ring_lds_bytes(int P, int nl, int slots);
int panel_ring_errors(const Matrix *m, hipStream_t s);
// the `form` and `unroll` of spl_matrix_build_panel (SPL_PANEL_FORM_*): known to these functions only
bool panel_code_valid(int form, int unroll);
bool panel_code_takes_slices(int form);
int panel_slices_override();  // SPL_PANEL_SLICES, 0: not set
PanelPlan panel_plan_from_code(int form, int unroll, int cols_log2, int nslices);
// the plan for a freshly built image: the code's plan, the register sets sized from the image when unroll is 0,
// and, for the all-default request on a large matrix (may_tune), the fastest of the heuristic's neighbours
PanelPlan choose_panel_plan(const Matrix *m, const PanelImage *b, int form, int unroll, int nslices, bool may_tune);
// choose the blocked image's shape for this matrix (0,0 = blocking would not help)
void choose_blocking(const Matrix *m, int *rows_per_panel, int *w, int *waves);
void choose_panels(const Matrix *m, int *rows_per_panel, int *w);
void choose_panels(const Matrix *m, int *rows_per_panel, int *w, int *nslices);
int spmv_kernel_in_use(const Matrix *m);
bool panels_pay(const Matrix *m);
bool panels_beat_stream(const Matrix *m);  // order-free mode: the panel image instead of the CSR-stream kernel

// ---- pivot products (determinant.hip) ---------------------------------------------------------
// product of |pivot| over the non-zero finite pivots = m 2^e (m in [0.5, 1)); neg / zero / bad: pivots < 0 / == 0 /
// inf or NaN
struct DetResult {
  double m;
  int64_t e;
  int64_t neg, zero, bad;
};
DetResult det_pivots_strided(int64_t n, const double *d_diag, int64_t stride, hipStream_t s);
DetResult det_pivots_tree(int64_t n, const double *d_arena, const int *d_front_of, const int *d_p0, const int *d_ldp,
                          const int64_t *d_poff, hipStream_t s);
// parity (0 / 1) of all row interchanges of the threshold pivoting inside diagonal blocks: slot[b] = offset of the stored
// inv(L11) P_b of block b in d_invs, jb[b] its pivots
int block_pivot_parity(const double *d_invs, const std::vector<int64_t> &slot, const std::vector<int> &jb, hipStream_t s);

}  // namespace spl

// abi.hip — the extern "C" surface declared in include/sparse_linear_hip.h.
// Host-side marshalling only; every numerical step runs in a HIP kernel.
#include <stdio.h>
#include <vector>

#include "common.hpp"

namespace spl {

static thread_local char g_last_error[512] = "";

void set_last_error(const char *where, hipError_t e) {
  snprintf(g_last_error, sizeof(g_last_error), "%s: %s", where, hipGetErrorString(e));
}
void set_last_error_text(const char *text) { snprintf(g_last_error, sizeof(g_last_error), "%s", text); }

namespace {

// run f(), mapping C++ failures to status codes
template <typename F>
int guarded(F &&f) {
  try {
    return f();
  } catch (const DeviceError &e) {
    return e.status;
  } catch (const std::bad_alloc &) {
    return SPL_ERROR_out_of_memory;
  } catch (...) {
    return SPL_ERROR_internal;
  }
}

int current_device() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    set_last_error_text("no HIP device visible");
    throw DeviceError{SPL_ERROR_device};
  }
  int dev = 0;
  SPL_HIP(hipGetDevice(&dev));
  return dev;
}

bool whole(const Matrix *m) { return m->row0 == 0 && m->nrows_local == m->nrows_global; }

// ---- what the entry points of the objects behind handles share -------------------------------------------------------
inline int device_of(const Matrix *m) { return m->device; }
template <typename T>
int device_of(const T *object) { return head(object).device; }

// spl_*_free: the object goes with its own device current, and the handle is cleared whatever it held
template <typename T>
void free_object(void **h, T *(*as)(void *), void (*destroy)(T *)) {
  if (!h || !*h) return;
  T *object = as(*h);
  *h = nullptr;
  if (!object) return;
  int prev = -1;
  const bool have_prev = hipGetDevice(&prev) == hipSuccess;
  (void)hipSetDevice(device_of(object));  // may run on a finalizer thread with another current device
  destroy(object);
  if (have_prev) (void)hipSetDevice(prev);
}

// the tail of an entry point that makes an object from the handle A, on A's device: make(&object) returns the status
template <typename T, typename Make>
int create_object(const Matrix *A, void **out, Make &&make) {
  return guarded([&]() -> int {
    (void)current_device();
    DeviceGuard g(A->device);
    T *object = nullptr;
    const int st = make(&object);
    *out = object;
    return st;
  });
}

// spl_*_info
template <typename T, typename P>
int info_of(void *h, T *(*as)(void *), void (*info_fn)(P *, int64_t *), int64_t info[8]) {
  T *object = as(h);
  if (!object) return SPL_ERROR_invalid_handle;
  if (!info) return SPL_ERROR_argument_missing;
  info_fn(object, info);
  return SPL_OK;
}

// a part serves an object of its size, value kind and device only
inline bool same_shape(const ObjectHead &a, const ObjectHead &b) {
  return a.n == b.n && a.vw == b.vw && a.device == b.device;
}

// spl_*_set_preconditioner: the triangular parts and the diagonal of a preconditioner for the solver behind h; the
// object behind T1 / T2, or nullptr for NULL (the identity), goes to set()
template <typename T>
int set_preconditioner_of(void *h, T *(*as)(void *), void (*set)(T *, TriSolver *, const double *, TriSolver *), void *T1,
                          const double *d_mid, void *T2) {
  T *S = as(h);
  if (!S) return SPL_ERROR_invalid_handle;
  void *given[2] = {T1, T2};
  TriSolver *parts[2] = {nullptr, nullptr};
  for (int i = 0; i < 2; ++i) {
    if (!given[i]) continue;
    parts[i] = as_trisolver(given[i]);
    if (!parts[i]) return SPL_ERROR_invalid_handle;
  }
  if ((uintptr_t)d_mid % (uintptr_t)(8 * head(S).vw) != 0) return SPL_ERROR_argument_missing;
  for (int i = 0; i < 2; ++i)
    if (parts[i] && !same_shape(head(parts[i]), head(S))) return SPL_ERROR_dimension_mismatch;
  set(S, parts[0], d_mid, parts[1]);
  return SPL_OK;
}

// spl_*_set_preconditioner_amg: M is borrowed and may serve several solvers; NULL takes the preconditioner away
template <typename T>
int set_preconditioner_amg_of(void *h, T *(*as)(void *), void (*set)(T *, Amg *), void *M) {
  T *S = as(h);
  if (!S) return SPL_ERROR_invalid_handle;
  Amg *P = nullptr;
  if (M) {
    P = as_amg(M);
    if (!P) return SPL_ERROR_invalid_handle;
    if (!same_shape(head(P), head(S))) return SPL_ERROR_dimension_mismatch;
  }
  set(S, P);
  return SPL_OK;
}

// what the solve calls of CG, BiCGSTAB and GMRES refuse before anything else is looked at; outputs: none of the
// arrays the results go to is NULL
int check_linear_solve(bool valid, bool outputs, double rtol, double atol, int64_t max_iter, int check_every,
                       const double *history) {
  if (!valid) return SPL_ERROR_invalid_handle;
  if (!outputs) return SPL_ERROR_argument_missing;
  if (max_iter < 0) return SPL_ERROR_n_nonpositive;
  if (!(rtol >= 0.0) || !(atol >= 0.0) || check_every < 0) return SPL_ERROR_argument_missing;  // a NaN is refused too
  if (history && max_iter >= ((int64_t)1 << 31)) return SPL_ERROR_index_overflow;
  return SPL_OK;
}
// the result of a solve with n == 0
void empty_linear_result(int nresult, int64_t *result, double *history) {
  for (int i = 0; i < nresult; ++i) result[i] = 0;
  if (history) history[0] = 0.0;
}

// the two device vectors of a solve or an application: given, apart, and aligned to whole entries (the kernels load
// and store whole entries)
int check_device_vectors(const ObjectHead &o, const double *d_b, const double *d_x) {
  if (!d_b || !d_x || d_b == d_x) return SPL_ERROR_argument_missing;
  const uintptr_t entry = (uintptr_t)(8 * o.vw);
  if ((uintptr_t)d_b % entry != 0 || (uintptr_t)d_x % entry != 0) return SPL_ERROR_argument_missing;
  return SPL_OK;
}

// The opening of spl_krylov_create, spl_gmres_create and spl_eigsh_create: A is a whole square handle, *out is
// cleared, option_ok says that the method / restart / ncv was in range
int square_whole_matrix(void *A, void **out, bool option_ok, Matrix **M) {
  *M = as_matrix(A);
  if (!*M) return SPL_ERROR_invalid_handle;
  if (!out) return SPL_ERROR_argument_missing;
  *out = nullptr;
  if (!option_ok) return SPL_ERROR_argument_missing;
  if ((*M)->nrows_global != (*M)->ncols) return SPL_ERROR_dimension_mismatch;
  if (!whole(*M)) return SPL_ERROR_invalid_matrix;
  return SPL_OK;
}

// The host-side entry points of the objects: a device block of `slots` vectors of `count` doubles on the object's
// device; up0 goes up to slot 0 and up1 (when given) to slot 1; run(block, stream) on the default stream; then slot
// `down_slot` comes down to `down` (nullptr: run enqueued its own copies) and the stream is synchronised
template <typename Run>
int with_host_vectors(int device, size_t count, size_t slots, const double *up0, const double *up1, size_t down_slot,
                      double *down, Run &&run) {
  return guarded([&]() -> int {
    DeviceGuard g(device);
    hipStream_t s = nullptr;
    DBuf<double> d(slots * count);
    SPL_HIP(hipMemcpyAsync(d.get(), up0, count * sizeof(double), hipMemcpyHostToDevice, s));
    if (up1) SPL_HIP(hipMemcpyAsync(d.get() + count, up1, count * sizeof(double), hipMemcpyHostToDevice, s));
    const int st = run(d.get(), s);
    if (st != SPL_OK) {
      (void)hipStreamSynchronize(s);
      return st;
    }
    if (down) SPL_HIP(hipMemcpyAsync(down, d.get() + down_slot * count, count * sizeof(double), hipMemcpyDeviceToHost, s));
    SPL_HIP(hipStreamSynchronize(s));
    return SPL_OK;
  });
}

// The same for the two eigensolvers: the k columns of `up`, ld entries apart, go up to the first k slots;
// run(block, vectors, stream) with `vectors` the nev slots behind them; then the result[3] columns found come down to
// `down`, ldx entries apart
template <typename Run>
int with_host_columns(const ObjectHead &o, int k, const double *up, int64_t ld, int nev, double *down, int64_t ldx,
                      const int64_t *result, Run &&run) {
  const size_t count = (size_t)o.n * (size_t)o.vw;
  return with_host_vectors(o.device, count, (size_t)k + (size_t)nev, up, nullptr, 0, nullptr, [&](double *d, hipStream_t s) {
    for (int j = 1; j < k; ++j)
      SPL_HIP(hipMemcpyAsync(d + (size_t)j * count, up + (size_t)j * (size_t)ld * (size_t)o.vw, count * sizeof(double),
                             hipMemcpyHostToDevice, s));
    double *d_vectors = d + (size_t)k * count;
    const int st = run(d, d_vectors, s);
    if (st != SPL_OK) return st;
    for (int64_t i = 0; i < result[3]; ++i)
      SPL_HIP(hipMemcpyAsync(down + (size_t)i * (size_t)ldx * (size_t)o.vw, d_vectors + (size_t)i * count,
                             count * sizeof(double), hipMemcpyDeviceToHost, s));
    return SPL_OK;
  });
}

// What the solve calls of Lanczos and LOBPCG refuse before the vectors are looked at.  columns: ncv or the block; the
// solve returns up to that less `spare` pairs, in one of the orders 0 ... which_most (SPL_EIGSH_*), and needs at least
// `least_rounds` restarts or iterations
template <typename T>
int check_eigen_solve(const T *S, int (*columns)(const T *), int spare, int which_most, int64_t least_rounds, int nev,
                      int which, double tol, double atol, int64_t rounds, const double *values, const double *residuals,
                      const int64_t *result, const double *history) {
  if (!S) return SPL_ERROR_invalid_handle;
  if (!values || !residuals || !result) return SPL_ERROR_argument_missing;
  if (rounds < least_rounds) return SPL_ERROR_n_nonpositive;
  if (nev < 1 || nev > columns(S) - spare || (int64_t)columns(S) > head(S).n || which < 0 || which > which_most ||
      !(tol >= 0.0) || !(atol >= 0.0))
    return SPL_ERROR_argument_missing;  // a NaN is refused too
  if (history && rounds >= ((int64_t)1 << 31)) return SPL_ERROR_index_overflow;
  return SPL_OK;
}

// spl_vector_rotate_dev and, with y_complex, spl_vector_rotate_z_dev: a complex Y makes a complex result
int rotate_checked(int64_t n, int value_width, int m, int k, double *d_V, int64_t ldv, const double *d_Y, int ldy,
                   double *d_out, int64_t ldo, void *stream, bool y_complex) {
  if (n < 0) return SPL_ERROR_n_nonpositive;
  if (value_width != 2 && (y_complex || value_width != 1)) return SPL_ERROR_argument_missing;
  if (m < 1 || m > 128 || k < 1 || k > m || ldv < n || ldy < m || (d_out && ldo < n)) return SPL_ERROR_argument_missing;
  if (n > 0 && (!d_V || !d_Y)) return SPL_ERROR_argument_missing;
  const uintptr_t entry = (uintptr_t)(8 * value_width);  // the kernel loads and stores whole entries; Y double by double
  if ((uintptr_t)d_V % entry != 0 || (uintptr_t)d_Y % sizeof(double) != 0 || (uintptr_t)d_out % entry != 0)
    return SPL_ERROR_argument_missing;
  if (d_out && n > 0) {  // the result beside V, not over it
    const uintptr_t v0 = (uintptr_t)d_V, v1 = v0 + ((uintptr_t)(m - 1) * (uintptr_t)ldv + (uintptr_t)n) * entry;
    const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + ((uintptr_t)(k - 1) * (uintptr_t)ldo + (uintptr_t)n) * entry;
    if (o0 < v1 && v0 < o1) return SPL_ERROR_argument_missing;
  }
  return guarded([&]() -> int {
    (void)current_device();
    return vector_rotate(n, value_width, m, k, d_V, ldv, d_Y, ldy, d_out, ldo, as_stream(stream), y_complex);
  });
}

template <typename T>
void upload(DBuf<T> &dst, const T *src, size_t n, hipStream_t s) {
  dst.alloc(n);
  if (n) SPL_HIP(hipMemcpyAsync(dst.get(), src, n * sizeof(T), hipMemcpyHostToDevice, s));
}

// malloc()'d host arrays, freed unless released to a caller who frees them with spl_free
struct FreeDeleter {
  void operator()(void *p) const { free(p); }
};
template <typename T>
using HostArray = std::unique_ptr<T[], FreeDeleter>;
template <typename T>
HostArray<T> host_alloc(size_t n) {
  return HostArray<T>(static_cast<T *>(malloc(n * sizeof(T))));
}

int check_tuple(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax) {
  if (nrows < 0 || ncols < 0) return SPL_ERROR_n_nonpositive;
  if (!Ap) return SPL_ERROR_argument_missing;
  const int nnz = Ap[ncols];
  if (nnz < 0) return SPL_ERROR_invalid_matrix;
  if (nnz > 0 && (!Ai || !Ax)) return SPL_ERROR_argument_missing;
  return SPL_OK;
}

// a CSC 5-tuple on the device; x holds vw doubles per entry (2: packed complex)
struct DeviceCsc {
  DBuf<int> p, i;
  DBuf<double> x;
  int64_t nnz = 0;
};

// upload a CSC 5-tuple that passed check_tuple and validate its pointers and indices
int upload_validated(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax, int vw, DeviceCsc &d,
                     hipStream_t s) {
  d.nnz = Ap[ncols];
  upload(d.p, Ap, (size_t)ncols + 1, s);
  upload(d.i, Ai, (size_t)d.nnz, s);
  upload(d.x, Ax, (size_t)d.nnz * (size_t)vw, s);
  return validate_compressed(d.p.get(), d.i.get(), ncols, nrows, d.nnz, s);
}

// check, upload and validate a CSC 5-tuple; sort its columns if a caller violated the ascending-row invariant
// (the reference's SPA does not care about input order)
int upload_csc(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax, int vw, DeviceCsc &d,
               hipStream_t s) {
  int st = check_tuple(nrows, ncols, Ap, Ai, Ax);
  if (st != SPL_OK) return st;
  st = upload_validated(nrows, ncols, Ap, Ai, Ax, vw, d, s);
  if (st != SPL_OK) return st;
  if (!columns_sorted(d.p.get(), d.i.get(), ncols, s)) {
    DBuf<int64_t> p64((size_t)ncols + 1);
    widen_i32_to_i64(d.p.get(), p64.get(), (int64_t)ncols + 1, s);
    if (vw == 1) {
      segmented_sort_pairs(p64.get(), ncols, d.i.get(), d.x.get(), s);
      SPL_HIP(hipStreamSynchronize(s));
    } else {
      // packed complex: sort the entry positions with the rows, then gather the 16-byte values along them
      DBuf<double> pos((size_t)d.nnz), sorted((size_t)d.nnz * 2);
      fill_positions(d.nnz, pos.get(), s);
      segmented_sort_pairs(p64.get(), ncols, d.i.get(), pos.get(), s);
      gather_complex_values(d.nnz, pos.get(), d.x.get(), sorted.get(), s);
      SPL_HIP(hipStreamSynchronize(s));
      d.x = std::move(sorted);
    }
  }
  return SPL_OK;
}

// copy a device CSC result into malloc()'d host arrays the caller adopts (`fromForeign False`, freed with spl_free);
// vw doubles per value
int download_result(int64_t ncols, int64_t nnz, int vw, const int64_t *dCp64, const int *dCi, const double *dCx,
                    int **Cp, int **Ci, double **Cx, hipStream_t s) {
  if (nnz >= 0x7fffffffLL) return SPL_ERROR_index_overflow;
  const size_t n = (size_t)(nnz ? nnz : 1);
  HostArray<int> hp = host_alloc<int>((size_t)ncols + 1), hi = host_alloc<int>(n);
  HostArray<double> hx = host_alloc<double>(n * (size_t)vw);
  if (!hp || !hi || !hx) return SPL_ERROR_out_of_memory;
  DBuf<int> dCp32((size_t)ncols + 1);
  narrow_i64_to_i32(dCp64, dCp32.get(), ncols + 1, s);
  SPL_HIP(hipMemcpyAsync(hp.get(), dCp32.get(), ((size_t)ncols + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
  if (nnz) {
    SPL_HIP(hipMemcpyAsync(hi.get(), dCi, (size_t)nnz * sizeof(int), hipMemcpyDeviceToHost, s));
    SPL_HIP(hipMemcpyAsync(hx.get(), dCx, (size_t)nnz * (size_t)vw * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  SPL_HIP(hipStreamSynchronize(s));
  *Cp = hp.release();
  *Ci = hi.release();
  *Cx = hx.release();
  return SPL_OK;
}

// a handle under construction: rows [row0, row0 + nrows_local) of an nrows_global x ncols matrix, vw doubles per value
std::unique_ptr<Matrix> make_matrix(int device, int64_t nrows_global, int64_t ncols, int64_t row0, int64_t nrows_local,
                                    int vw = 1) {
  std::unique_ptr<Matrix> m(new Matrix());
  m->device = device;
  m->nrows_global = nrows_global;
  m->ncols = ncols;
  m->row0 = row0;
  m->nrows_local = nrows_local;
  m->vw = vw;
  return m;
}

// An nrows x ncols CSC tuple that upload_csc (columns sorted) or upload_validated (columns as they are) put on the
// device, as an unpublished handle: its arrays, unchanged, are the ROW image of the transpose (ncols rows, nrows
// columns).  What kronecker_handles, assemble_handles and take_diag_handle read is filled (rowptr64 / colidx / val / nnz,
// the dimensions, vw); the handle is not finalized.  The arrays move out of d.
std::unique_ptr<Matrix> transposed_image(int device, int nrows, int ncols, int vw, DeviceCsc &d, hipStream_t s) {
  std::unique_ptr<Matrix> m = make_matrix(device, ncols, nrows, 0, ncols, vw);
  m->nnz = d.nnz;
  m->rowptr64.alloc((size_t)ncols + 1);
  widen_i32_to_i64(d.p.get(), m->rowptr64.get(), (int64_t)ncols + 1, s);
  m->rowptr = std::move(d.p);
  m->colidx = std::move(d.i);
  m->val = std::move(d.x);
  return m;
}

// finish a handle whose rowptr64 / colidx / val are filled and hand it to the caller
int publish(std::unique_ptr<Matrix> m, hipStream_t s, void **H) {
  finalize_matrix(m.get(), s);
  *H = m.release();
  return SPL_OK;
}

// Build the row-major image of a CSC 5-tuple with vw doubles per value on the current device (not yet finalized).
// out receives rows [row0,row1) chosen as the part-th of nparts nnz-balanced blocks; packed complex tuples come
// whole (nparts == 1).
int build_from_csc(int vw, int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax, int part, int nparts,
                   std::unique_ptr<Matrix> &out) {
  int st = check_tuple(nrows, ncols, Ap, Ai, Ax);
  if (st != SPL_OK) return st;
  if (nparts < 1 || part < 0 || part >= nparts) return SPL_ERROR_argument_missing;
  const int dev = current_device();
  hipStream_t s = nullptr;
  DeviceCsc A;
  st = upload_validated(nrows, ncols, Ap, Ai, Ax, vw, A, s);
  if (st != SPL_OK) return st;
  const int64_t nnz = A.nnz;

  std::unique_ptr<Matrix> full = make_matrix(dev, nrows, ncols, 0, nrows, vw);
  full->nnz = nnz;
  if (vw == 1) {
    full->rowptr64.alloc((size_t)nrows + 1);
    full->colidx.alloc((size_t)nnz);
    full->val.alloc((size_t)nnz);
    transpose_compressed(A.p.get(), A.i.get(), A.x.get(), ncols, nrows, nnz, full->rowptr64.get(), full->colidx.get(),
                         full->val.get(), s);
  } else {
    // packed complex (Umfpack/Internal.hs:124-132): transpose the PATTERN with the entry positions as payload and
    // gather the 16-byte values along the permutation
    DBuf<double> pos((size_t)nnz), perm((size_t)nnz);
    fill_positions(nnz, pos.get(), s);
    full->rowptr64.alloc((size_t)nrows + 1);
    full->colidx.alloc((size_t)nnz);
    full->val.alloc((size_t)nnz * 2);
    transpose_compressed(A.p.get(), A.i.get(), pos.get(), ncols, nrows, nnz, full->rowptr64.get(), full->colidx.get(),
                         perm.get(), s);
    gather_complex_values(nnz, perm.get(), A.x.get(), full->val.get(), s);
    SPL_HIP(hipStreamSynchronize(s));
  }
  if (nparts == 1) {
    out = std::move(full);
    return SPL_OK;
  }
  // nnz-balanced contiguous row blocks: block p starts at the first row whose
  // pointer is >= nnz*p/nparts (identical on every rank: same input, same rule)
  std::vector<int64_t> hptr((size_t)nrows + 1);
  SPL_HIP(hipMemcpy(hptr.data(), full->rowptr64.get(), ((size_t)nrows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
  auto boundary = [&](int p) -> int64_t {
    if (p <= 0) return 0;
    if (p >= nparts) return nrows;
    const int64_t target = (int64_t)(((__int128)nnz * p) / nparts);
    int64_t lo = 0, hi = nrows;
    while (lo < hi) {
      const int64_t mid = (lo + hi) / 2;
      if (hptr[(size_t)mid] < target) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  const int64_t r0 = boundary(part), r1 = boundary(part + 1);
  std::unique_ptr<Matrix> blk = make_matrix(dev, nrows, ncols, r0, r1 - r0);
  const int64_t k0 = hptr[(size_t)r0], k1 = hptr[(size_t)r1];
  blk->nnz = k1 - k0;
  std::vector<int64_t> rel((size_t)(r1 - r0) + 1);
  for (int64_t i = 0; i <= r1 - r0; ++i) rel[(size_t)i] = hptr[(size_t)(r0 + i)] - k0;
  upload(blk->rowptr64, rel.data(), rel.size(), s);
  blk->colidx.alloc((size_t)blk->nnz);
  blk->val.alloc((size_t)blk->nnz);
  if (blk->nnz) {
    SPL_HIP(hipMemcpyAsync(blk->colidx.get(), full->colidx.get() + k0, (size_t)blk->nnz * sizeof(int),
                           hipMemcpyDeviceToDevice, s));
    SPL_HIP(hipMemcpyAsync(blk->val.get(), full->val.get() + k0, (size_t)blk->nnz * sizeof(double),
                           hipMemcpyDeviceToDevice, s));
  }
  SPL_HIP(hipStreamSynchronize(s));
  out = std::move(blk);
  return SPL_OK;
}

// the finalized image of a real CSC 5-tuple, for the one-shot SpMV / SpMM calls
int one_shot_image(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax, std::unique_ptr<Matrix> &m) {
  int st = build_from_csc(1, nrows, ncols, Ap, Ai, Ax, 0, 1, m);
  if (st == SPL_OK) finalize_matrix(m.get(), nullptr);
  return st;
}

// a CSC 5-tuple as the caller passed it
struct HostCsc {
  int nrows, ncols;
  const int *p, *i;
  const double *x;
};

// a device result with 64-bit column pointers, as the SpGEMM / lin / kron kernels produce it
struct DeviceResult {
  DBuf<int64_t> p;
  DBuf<int> i;
  DBuf<double> x;
  int64_t nnz = 0;
};

// the body of the one-shot binary operations (spl_spgemm, spl_lin, spl_kronecker and their complex forms), after the
// caller's argument checks: upload A and B with vw doubles per value, op(A, B, C, s) on the device (it may refuse with
// a status before it allocates anything of C), download the nrowsC x ncolsC result into the caller's *Cp / *Ci / *Cx;
// the shape is written on success only
template <typename Op>
int binary_one_shot(int vw, const HostCsc &a, const HostCsc &b, int64_t nrowsC, int64_t ncolsC, int *nrowsC_out,
                    int *ncolsC_out, int **Cp, int **Ci, double **Cx, Op &&op) {
  return guarded([&]() -> int {
    (void)current_device();
    hipStream_t s = nullptr;
    DeviceCsc A, B;
    int st = upload_csc(a.nrows, a.ncols, a.p, a.i, a.x, vw, A, s);
    if (st != SPL_OK) return st;
    st = upload_csc(b.nrows, b.ncols, b.p, b.i, b.x, vw, B, s);
    if (st != SPL_OK) return st;
    DeviceResult C;
    st = op(A, B, C, s);
    if (st != SPL_OK) return st;
    st = download_result(ncolsC, C.nnz, vw, C.p.get(), C.i.get(), C.x.get(), Cp, Ci, Cx, s);
    if (st != SPL_OK) return st;
    *nrowsC_out = (int)nrowsC;
    *ncolsC_out = (int)ncolsC;
    return SPL_OK;
  });
}

// y (host) = A x (host) [+ y]
int host_spmv(Matrix *m, int xlen, const double *x, int ylen, double *y, int accumulate) {
  if ((int64_t)xlen != m->ncols) return SPL_ERROR_dimension_mismatch;     // Sparse.hs:438-441
  if ((int64_t)ylen != m->nrows_local) return SPL_ERROR_dimension_mismatch;  // Sparse.hs:442-445
  if ((xlen > 0 && !x) || (ylen > 0 && !y)) return SPL_ERROR_argument_missing;
  DeviceGuard g(m->device);
  hipStream_t s = nullptr;
  DBuf<double> dx, dy;
  const size_t vw = (size_t)m->vw;  // packed complex vectors carry two doubles per entry
  upload(dx, x, (size_t)xlen * vw, s);
  if (accumulate) upload(dy, y, (size_t)ylen * vw, s); else dy.alloc((size_t)ylen * vw);
  int st = launch_spmv(m, dx.get(), dy.get(), accumulate, s);
  if (st != SPL_OK) return st;
  if (ylen) SPL_HIP(hipMemcpyAsync(y, dy.get(), (size_t)ylen * vw * sizeof(double), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  return SPL_OK;
}

}  // namespace
}  // namespace spl

using namespace spl;

extern "C" {

const char *spl_status_string(int status) {
  switch (status) {
    case SPL_OK: return "OK";
    case SPL_WARNING_singular_matrix: return "warning: singular matrix";
    case SPL_ERROR_out_of_memory: return "out of memory";
    case SPL_ERROR_invalid_handle: return "invalid handle";
    case SPL_ERROR_argument_missing: return "argument missing or invalid";
    case SPL_ERROR_n_nonpositive: return "negative dimension";
    case SPL_ERROR_invalid_matrix: return "invalid matrix (pointers not monotone or index out of range)";
    case SPL_ERROR_dimension_mismatch: return "dimension mismatch";
    case SPL_ERROR_index_out_of_bounds: return "index out of bounds";
    case SPL_ERROR_index_overflow: return "result does not fit 32-bit indices";
    case SPL_ERROR_device: return "HIP device error";
    case SPL_ERROR_internal: return "internal error";
    default: return "unknown status";
  }
}

int spl_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char *spl_last_error(void) { return g_last_error; }

void spl_free(void *p) { free(p); }

unsigned long long spl_release_cached_memory(void) { return (unsigned long long)device_release_cached(); }

double spl_device_alloc_seconds(void) { return device_alloc_seconds(); }

int spl_matrix_create(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax, void **H) {
  return spl_matrix_create_rowblock(nrows, ncols, Ap, Ai, Ax, 0, 1, H);
}

int spl_matrix_create_rowblock(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax,
                               int part, int nparts, void **H) {
  if (!H) return SPL_ERROR_argument_missing;
  *H = nullptr;
  return guarded([&]() -> int {
    std::unique_ptr<Matrix> m;
    int st = build_from_csc(1, nrows, ncols, Ap, Ai, Ax, part, nparts, m);
    return st != SPL_OK ? st : publish(std::move(m), nullptr, H);
  });
}

// Complex Double: the CSC 5-tuple with packed (re, im) values (what the reference passes for its complex
// instance, Umfpack/Internal.hs:124-132)
int spl_matrix_create_z(int nrows, int ncols, const int *Ap, const int *Ai, const double *Az, void **H) {
  if (!H) return SPL_ERROR_argument_missing;
  *H = nullptr;
  return guarded([&]() -> int {
    std::unique_ptr<Matrix> m;
    int st = build_from_csc(2, nrows, ncols, Ap, Ai, Az, 0, 1, m);
    return st != SPL_OK ? st : publish(std::move(m), nullptr, H);
  });
}

int spl_matrix_is_complex(void *H) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  return m->vw == 2 ? 1 : 0;
}

int spl_matrix_create_csr(int64_t nrows_global, int64_t ncols, int64_t row0, int64_t nrows_local,
                          const int *rowptr, const int *colidx, const double *val, void **H) {
  if (!H) return SPL_ERROR_argument_missing;
  *H = nullptr;
  if (nrows_global < 0 || ncols < 0 || nrows_local < 0 || row0 < 0) return SPL_ERROR_n_nonpositive;
  if (row0 + nrows_local > nrows_global || ncols > 0x7fffffffLL) return SPL_ERROR_argument_missing;
  if (!rowptr) return SPL_ERROR_argument_missing;
  const int64_t nnz = rowptr[nrows_local];
  if (nnz < 0) return SPL_ERROR_invalid_matrix;
  if (nnz > 0 && (!colidx || !val)) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    const int dev = current_device();
    hipStream_t s = nullptr;
    std::unique_ptr<Matrix> m = make_matrix(dev, nrows_global, ncols, row0, nrows_local);
    m->nnz = nnz;
    DBuf<int> dptr;
    upload(dptr, rowptr, (size_t)nrows_local + 1, s);
    upload(m->colidx, colidx, (size_t)nnz, s);
    upload(m->val, val, (size_t)nnz, s);
    int st = validate_compressed(dptr.get(), m->colidx.get(), nrows_local, ncols, nnz, s);
    if (st != SPL_OK) return st;
    m->rowptr64.alloc((size_t)nrows_local + 1);
    widen_i32_to_i64(dptr.get(), m->rowptr64.get(), nrows_local + 1, s);
    // rows with unsorted columns are tolerated as unsorted CSC columns are (upload_csc): lin, spgemm, the transposes
    // and the reference-order SpMV all walk ascending indices.  A sorted input pays the check only.
    if (!columns_sorted(dptr.get(), m->colidx.get(), nrows_local, s)) {
      segmented_sort_pairs(m->rowptr64.get(), nrows_local, m->colidx.get(), m->val.get(), s);
      SPL_HIP(hipStreamSynchronize(s));
    }
    return publish(std::move(m), s, H);
  });
}

int spl_matrix_create_synthetic(int kind, int64_t n_or_m, int K, uint64_t seed, int64_t row0,
                                int64_t row1, void **H) {
  if (!H) return SPL_ERROR_argument_missing;
  *H = nullptr;
  if (kind < 0 || kind > 3 || n_or_m <= 0) return SPL_ERROR_argument_missing;
  if (kind == 0 && (K < 1 || K > 64)) return SPL_ERROR_argument_missing;
  int64_t n = n_or_m;
  if (kind == 2) n = n_or_m * n_or_m;
  if (kind == 3) n = n_or_m * n_or_m * n_or_m;
  if (n > 0x7fffffffLL) return SPL_ERROR_index_overflow;
  if (row0 < 0 || row1 < row0 || row1 > n) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    std::unique_ptr<Matrix> m = make_matrix(current_device(), n, n, row0, row1 - row0);
    generate_synthetic(m.get(), kind, n_or_m, K, seed, nullptr);
    return publish(std::move(m), nullptr, H);
  });
}

int spl_matrix_create_rmat(int scale, int edge_factor, double a, double b, double c, uint64_t seed,
                           void **H) {
  if (!H) return SPL_ERROR_argument_missing;
  *H = nullptr;
  if (scale < 1 || scale > 30 || edge_factor < 1 || a < 0 || b < 0 || c < 0 || a + b + c > 1.0)
    return SPL_ERROR_argument_missing;
  const int64_t n = 1LL << scale;
  const int64_t nedges = n * edge_factor;
  if (nedges >= 0x7fffffffLL) return SPL_ERROR_index_overflow;
  return guarded([&]() -> int {
    const int dev = current_device();
    hipStream_t s = nullptr;
    auto thr = [](double p) -> uint32_t {
      const double v = p * 4294967296.0;
      return v >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)v;
    };
    DBuf<int> dr((size_t)nedges), dc((size_t)nedges), dptr((size_t)n + 1), oidx;
    DBuf<double> dv((size_t)nedges), oval;
    generate_rmat_coo(seed, scale, thr(a), thr(a + b), thr(a + b + c), nedges, dr.get(), dc.get(), dv.get(), s);
    // row-major image: compress with the roles of rows and columns exchanged
    int64_t nz = 0, bad = -1;
    int st = compress_device((int)n, (int)n, nedges, dc.get(), dr.get(), dv.get(), dptr.get(), oidx, oval, &nz,
                             &bad, s);
    if (st != SPL_OK) return st;
    std::unique_ptr<Matrix> m = make_matrix(dev, n, n, 0, n);
    m->nnz = nz;
    m->rowptr64.alloc((size_t)n + 1);
    widen_i32_to_i64(dptr.get(), m->rowptr64.get(), n + 1, s);
    m->colidx = std::move(oidx);
    m->val = std::move(oval);
    return publish(std::move(m), s, H);
  });
}

int spl_matrix_spgemm(void *HA, void *HB, void **HC, int64_t *products) {
  Matrix *A = as_matrix(HA), *B = as_matrix(HB);
  if (!A || !B) return SPL_ERROR_invalid_handle;
  if (!HC) return SPL_ERROR_argument_missing;
  *HC = nullptr;
  if (A->vw != B->vw) return SPL_ERROR_argument_missing;  // one real, one complex: spl_matrix_to_complex first
  if (A->ncols != B->nrows_global || B->row0 != 0 || B->nrows_local != B->nrows_global)
    return SPL_ERROR_dimension_mismatch;  // Sparse.hs:694 (B must be whole; A may be a row block)
  if (!A->rowptr.get() || !B->rowptr.get()) return SPL_ERROR_index_overflow;
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    hipStream_t s = nullptr;
    std::unique_ptr<Matrix> C = make_matrix(A->device, A->nrows_global, B->ncols, A->row0, A->nrows_local, A->vw);
    // rows of A*B = columns of (A*B)^T = B^T * A^T: the CSR arrays of B and A are the CSC
    // arrays of B^T and A^T, so the column-wise kernel runs on them unchanged
    if (A->vw == 1)
      spgemm_device(B->ncols, B->nrows_global, B->rowptr.get(), B->colidx.get(), B->val.get(), A->nrows_local,
                    A->rowptr.get(), A->colidx.get(), A->val.get(), C->rowptr64, C->colidx, C->val, &C->nnz,
                    products, s);
    else  // the value kernel then forms b * a for the reference's a * b: the same bits, every operation rounded once
      spgemm_device_z(B->ncols, B->nrows_global, B->rowptr.get(), B->colidx.get(), B->val.get(), A->nrows_local,
                      A->rowptr.get(), A->colidx.get(), A->val.get(), C->rowptr64, C->colidx, C->val, &C->nnz,
                      products, s);
    return publish(std::move(C), s, HC);
  });
}

// ---- device-resident forms of lin / transpose / compress (round 3) -----------------------------------------
// The host 5-tuple entry points (spl_lin, spl_transpose, spl_compress) pay PCIe and marshalling for kernels that
// take a few milliseconds; these work handle to handle.  A handle holds the ROW-major image; `lin` merges along
// the major index whichever it is (Sparse.hs:401-431 applied to the transposes), so the same kernels serve.
int spl_matrix_lin(void *HA, const double alpha[2], void *HB, const double beta[2], void **HC) {
  Matrix *A = as_matrix(HA), *B = as_matrix(HB);
  if (!A || !B) return SPL_ERROR_invalid_handle;
  if (!HC || !alpha || !beta) return SPL_ERROR_argument_missing;
  *HC = nullptr;
  if (A->nrows_global != B->nrows_global || A->ncols != B->ncols || A->row0 != B->row0 || A->nrows_local != B->nrows_local)
    return SPL_ERROR_dimension_mismatch;  // Sparse.hs:408-409
  if (A->vw != B->vw || A->device != B->device) return SPL_ERROR_argument_missing;
  if (A->vw == 1 && (alpha[1] != 0.0 || beta[1] != 0.0)) return SPL_ERROR_argument_missing;  // complex scalars: spl_matrix_to_complex first
  if (!A->rowptr.get() || !B->rowptr.get()) return SPL_ERROR_index_overflow;
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    hipStream_t s = nullptr;
    std::unique_ptr<Matrix> C = make_matrix(A->device, A->nrows_global, A->ncols, A->row0, A->nrows_local, A->vw);
    if (A->vw == 1)
      lin_device(alpha[0], A->rowptr.get(), A->colidx.get(), A->val.get(), beta[0], B->rowptr.get(), B->colidx.get(),
                 B->val.get(), A->nrows_local, C->rowptr64, C->colidx, C->val, &C->nnz, s);
    else
      lin_device_z(alpha, A->rowptr.get(), A->colidx.get(), A->val.get(), beta, B->rowptr.get(), B->colidx.get(),
                   B->val.get(), A->nrows_local, C->rowptr64, C->colidx, C->val, &C->nnz, s);
    return publish(std::move(C), s, HC);
  });
}

namespace {
__global__ __launch_bounds__(256) void promote_complex_kernel(const double *__restrict__ x, int64_t n, double *__restrict__ z) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) { z[2 * i] = x[i]; z[2 * i + 1] = 0.0; }  // cmap (:+ 0)
}
}  // namespace

// the Complex Double handle of a real one: same pattern, values (x :+ 0)
int spl_matrix_to_complex(void *H, void **HZ) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if (!HZ) return SPL_ERROR_argument_missing;
  *HZ = nullptr;
  if (A->vw != 1) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    hipStream_t s = nullptr;
    std::unique_ptr<Matrix> C = make_matrix(A->device, A->nrows_global, A->ncols, A->row0, A->nrows_local, 2);
    C->nnz = A->nnz;
    C->rowptr64.alloc((size_t)A->nrows_local + 1);
    SPL_HIP(hipMemcpyAsync(C->rowptr64.get(), A->rowptr64.get(), ((size_t)A->nrows_local + 1) * sizeof(int64_t),
                           hipMemcpyDeviceToDevice, s));
    C->colidx.alloc((size_t)A->nnz);
    C->val.alloc((size_t)A->nnz * 2);
    if (A->nnz) {
      SPL_HIP(hipMemcpyAsync(C->colidx.get(), A->colidx.get(), (size_t)A->nnz * sizeof(int), hipMemcpyDeviceToDevice, s));
      int64_t blocks = (A->nnz + 255) / 256;
      if (blocks > 65536) blocks = 65536;
      hipLaunchKernelGGL(promote_complex_kernel, dim3((unsigned)blocks), dim3(256), 0, s, A->val.get(), A->nnz, C->val.get());
    }
    return publish(std::move(C), s, HZ);
  });
}

namespace {
// handle of the transpose of a whole matrix, real or complex (Sparse.hs:301-329 on the device, no host round trip);
// conjugate: of the conjugate transpose (Sparse.hs:371-375), which on a real handle is the same thing
int transpose_handle(void *H, void **HT, bool conjugate) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if (!HT) return SPL_ERROR_argument_missing;
  *HT = nullptr;
  if (A->row0 != 0 || A->nrows_local != A->nrows_global) return SPL_ERROR_argument_missing;
  if (!A->rowptr.get()) return SPL_ERROR_index_overflow;
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    hipStream_t s = nullptr;
    std::unique_ptr<Matrix> C = make_matrix(A->device, A->ncols, A->nrows_global, 0, A->ncols, A->vw);
    C->nnz = A->nnz;
    C->rowptr64.alloc((size_t)A->ncols + 1);
    C->colidx.alloc((size_t)A->nnz);
    C->val.alloc((size_t)A->nnz * (size_t)A->vw);
    if (A->vw == 1) {
      transpose_compressed(A->rowptr.get(), A->colidx.get(), A->val.get(), A->nrows_local, A->ncols, A->nnz,
                           C->rowptr64.get(), C->colidx.get(), C->val.get(), s);
    } else {
      // packed complex, as build_from_csc: transpose the pattern with the entry positions as payload, then gather
      // the 16-byte values along the permutation — conjugating them in that pass when asked to
      DBuf<double> pos((size_t)A->nnz), perm((size_t)A->nnz);
      fill_positions(A->nnz, pos.get(), s);
      transpose_compressed(A->rowptr.get(), A->colidx.get(), pos.get(), A->nrows_local, A->ncols, A->nnz,
                           C->rowptr64.get(), C->colidx.get(), perm.get(), s);
      gather_complex_values(A->nnz, perm.get(), A->val.get(), C->val.get(), s, conjugate);
      SPL_HIP(hipStreamSynchronize(s));  // perm is released on return
    }
    return publish(std::move(C), s, HT);
  });
}
}  // namespace

int spl_matrix_transpose(void *H, void **HT) { return transpose_handle(H, HT, false); }

int spl_matrix_ctrans(void *H, void **HC) { return transpose_handle(H, HC, true); }

// hermitian m = ctrans m == m (Sparse.hs:377-379) without building ctrans m (hermitian.hip); synchronises
int spl_matrix_hermitian(void *H, int *result) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if (!result || A->row0 != 0 || A->nrows_local != A->nrows_global) return SPL_ERROR_argument_missing;
  if (!A->rowptr.get()) return SPL_ERROR_index_overflow;
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    *result = hermitian_device(A, nullptr);
    return SPL_OK;
  });
}

// ---- the structural constructors, handle to handle (csrc/assemble_handles.hip) ------------------------------------
// C = A (x) B (`kronecker`, Sparse.hs:597-634).  A handle holds the ROW-major image, i.e. the CSC fields of the
// transpose, and (A (x) B)^T = A^T (x) B^T: the reference's walk — for every entry of A's column, every entry of B's,
// index ia * nrowsB + ib, value b * a — applied to the two row images writes the row image of A (x) B, so the handle
// that comes out is the reference's result, structure and values.
int spl_matrix_kronecker(void *HA, void *HB, void **HC) {
  Matrix *A = as_matrix(HA), *B = as_matrix(HB);
  if (!A || !B) return SPL_ERROR_invalid_handle;
  if (!HC) return SPL_ERROR_argument_missing;
  *HC = nullptr;
  if (!whole(A) || !whole(B)) return SPL_ERROR_argument_missing;
  if (A->vw != B->vw || A->device != B->device) return SPL_ERROR_argument_missing;  // spl_matrix_to_complex first
  const int64_t nrowsC = A->nrows_global * B->nrows_global, ncolsC = A->ncols * B->ncols;  // both factors < 2^31
  if (nrowsC >= 0x80000000LL || ncolsC >= 0x80000000LL) return SPL_ERROR_index_overflow;
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    hipStream_t s = nullptr;
    std::unique_ptr<Matrix> C = make_matrix(A->device, nrowsC, ncolsC, 0, nrowsC, A->vw);
    kronecker_handles(A, B, C.get(), s);
    return publish(std::move(C), s, HC);
  });
}

// hcat / vcat / fromBlocks / fromBlocksDiag / blockDiag (Sparse.hs:500-595, 661-667) as one placement of blocks.  In the
// reference column c of the result is the blocks' columns one after the other by ascending row offset; on the row
// images the same holds with rows and columns exchanged: row r is the rows of the blocks that cover it by ascending
// COLUMN offset.  The rectangles are disjoint, so either way every entry lands where the reference puts it.
int spl_matrix_assemble_blocks(int nblocks, void *const *H, const int64_t *row_off, const int64_t *col_off,
                               int64_t nrowsC, int64_t ncolsC, void **HC) {
  if (nblocks < 0) return SPL_ERROR_n_nonpositive;
  if (nblocks > 0 && !H) return SPL_ERROR_argument_missing;
  std::vector<const Matrix *> blk((size_t)nblocks);
  for (int b = 0; b < nblocks; ++b)
    if (!(blk[(size_t)b] = as_matrix(H[b]))) return SPL_ERROR_invalid_handle;
  if (!HC || (nblocks > 0 && (!row_off || !col_off))) return SPL_ERROR_argument_missing;
  *HC = nullptr;
  if (nrowsC < 0 || ncolsC < 0) return SPL_ERROR_n_nonpositive;
  for (int b = 0; b < nblocks; ++b) {
    if (!whole(blk[(size_t)b])) return SPL_ERROR_argument_missing;
    if (blk[(size_t)b]->vw != blk[0]->vw || blk[(size_t)b]->device != blk[0]->device) return SPL_ERROR_argument_missing;
  }
  if (nrowsC >= 0x80000000LL || ncolsC >= 0x80000000LL) return SPL_ERROR_index_overflow;
  std::vector<int> cut, lptr, list;
  const int st = blocks_table(nblocks, blk.data(), row_off, col_off, nrowsC, ncolsC, cut, lptr, list);
  if (st != SPL_OK) return st;
  return guarded([&]() -> int {
    const int dev = nblocks > 0 ? blk[0]->device : current_device();  // no block: `zeros` on the current device
    DeviceGuard g(dev);
    hipStream_t s = nullptr;
    std::unique_ptr<Matrix> C = make_matrix(dev, nrowsC, ncolsC, 0, nrowsC, nblocks > 0 ? blk[0]->vw : 1);
    assemble_handles(nblocks, blk.data(), row_off, col_off, cut, lptr, list, C.get(), s);
    return publish(std::move(C), s, HC);
  });
}

// d_out[c] = A[c, c] or 0 (`takeDiag`, Sparse.hs:640-650): the diagonal of the row image is the diagonal
int spl_matrix_take_diag_dev(void *H, double *d_out, void *stream) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if (!whole(A)) return SPL_ERROR_argument_missing;
  const int64_t n = A->nrows_global < A->ncols ? A->nrows_global : A->ncols;
  if (n > 0 && !d_out) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    take_diag_handle(A, n, d_out, as_stream(stream));
    return SPL_OK;
  });
}

// `diag` (Sparse.hs:652-659) of n values in device memory; without values `ident n` (Sparse.hs:669-671)
int spl_matrix_diag_dev(int64_t n, const double *d_values, int value_width, void **H) {
  if (!H) return SPL_ERROR_argument_missing;
  *H = nullptr;
  if (n < 0) return SPL_ERROR_n_nonpositive;
  if (value_width != 1 && value_width != 2) return SPL_ERROR_argument_missing;
  if (n >= 0x80000000LL) return SPL_ERROR_index_overflow;
  return guarded([&]() -> int {
    const int dev = current_device();
    hipStream_t s = nullptr;
    std::unique_ptr<Matrix> C = make_matrix(dev, n, n, 0, n, value_width);
    diag_handle(d_values, C.get(), s);
    return publish(std::move(C), s, H);
  });
}

// COO triples in device memory -> handle (compress / fromTriples, Sparse.hs:184-280: bounds checked rows first,
// then columns; duplicates summed in input order).  *bad receives the first offending position on
// SPL_ERROR_index_out_of_bounds (may be NULL).
int spl_matrix_compress_dev(int nrows, int ncols, int64_t ntriples, const int *d_rows, const int *d_cols,
                            const double *d_vals, void **H, int64_t *bad) {
  if (!H) return SPL_ERROR_argument_missing;
  *H = nullptr;
  if (nrows < 0 || ncols < 0) return SPL_ERROR_n_nonpositive;
  if (ntriples < 0 || (ntriples > 0 && (!d_rows || !d_cols || !d_vals))) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    const int dev = current_device();
    hipStream_t s = nullptr;
    // the row-major image of A is the column-major image of A^T: compress with the roles of rows and columns
    // exchanged.  The reference checks rows before columns (Sparse.hs:196-212): keep its order of complaints.
    {
      DBuf<int> none_i;
      DBuf<double> none_v;
      DBuf<int> probe((size_t)ncols + 1);
      int64_t nz = 0, where = -1;
      int st = compress_device(nrows, ncols, ntriples, d_rows, d_cols, d_vals, probe.get(), none_i, none_v, &nz, &where, s,
                               /*check_only=*/true);
      if (st != SPL_OK) { if (bad) *bad = where; return st; }
    }
    std::unique_ptr<Matrix> C = make_matrix(dev, nrows, ncols, 0, nrows);
    DBuf<int> ptr32((size_t)nrows + 1);
    int64_t where = -1;
    int st = compress_device(ncols, nrows, ntriples, d_cols, d_rows, d_vals, ptr32.get(), C->colidx, C->val, &C->nnz, &where, s, false);
    if (st != SPL_OK) { if (bad) *bad = where; return st; }
    C->rowptr64.alloc((size_t)nrows + 1);
    widen_i32_to_i64(ptr32.get(), C->rowptr64.get(), (int64_t)nrows + 1, s);
    return publish(std::move(C), s, H);
  });
}

// ---- compressed arrays and triples that are already in device memory (csrc/device_arrays.hip) ---------------------
namespace {

bool aligned_to(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the argument ladder the three imports share, everything that can be said before the device is touched
int import_arguments(int64_t nrows, int64_t ncols, int64_t count, int index_width, int value_width, void **H) {
  if (!H) return SPL_ERROR_argument_missing;
  *H = nullptr;
  if (nrows < 0 || ncols < 0 || count < 0) return SPL_ERROR_n_nonpositive;
  if (nrows >= 0x80000000LL || ncols >= 0x80000000LL) return SPL_ERROR_index_overflow;
  if ((index_width != 4 && index_width != 8) || (value_width != 1 && value_width != 2)) return SPL_ERROR_argument_missing;
  return SPL_OK;
}

// A checked, narrowed copy of compressed device arrays: nmajor slices over nminor indices.  ascending == nullptr: the
// order inside the slices is not looked at.  Values are not touched.
struct ImportedPattern {
  DBuf<int64_t> p64;
  DBuf<int> idx;
  int64_t nnz = 0;
};
int import_pattern(int index_width, const void *d_ptr, const void *d_idx, const double *d_val, int vw, int64_t nmajor,
                   int64_t nminor, bool csc, ImportedPattern &out, bool *ascending, hipStream_t s) {
  out.p64.alloc((size_t)nmajor + 1);
  out.nnz = import_pointers(index_width, d_ptr, nmajor, out.p64.get(), s);
  if (out.nnz < 0) return SPL_ERROR_invalid_matrix;
  if (out.nnz > 0 && (!d_idx || !d_val)) return SPL_ERROR_argument_missing;
  if (out.nnz == 0) {
    out.idx.alloc(0);
    return SPL_OK;
  }
  // a last pointer that promises more than the caller's allocations hold is refused before a byte of them is read
  if (out.nnz >= (1LL << 48) || !device_range_holds(d_idx, (size_t)out.nnz * (size_t)index_width) ||
      !device_range_holds(d_val, (size_t)out.nnz * (size_t)vw * sizeof(double)))
    return SPL_ERROR_invalid_matrix;
  if (csc && out.nnz >= 0x7fffffffLL) return SPL_ERROR_index_overflow;  // the transpose walks int32 pointers (export_csc)
  out.idx.alloc((size_t)out.nnz);
  return import_indices(index_width, d_idx, out.nnz, nminor, out.p64.get(), nmajor, out.idx.get(), ascending, s);
}

// sort the rows of m that do not ascend, values of m->vw doubles along with their indices
void sort_rows(Matrix *m, hipStream_t s) {
  if (m->vw == 1) {
    segmented_sort_pairs(m->rowptr64.get(), m->nrows_local, m->colidx.get(), m->val.get(), s);
  } else {
    // packed complex, as upload_csc: sort the entry positions with the indices, gather the 16-byte values along them
    DBuf<double> pos((size_t)m->nnz), sorted((size_t)m->nnz * 2);
    fill_positions(m->nnz, pos.get(), s);
    segmented_sort_pairs(m->rowptr64.get(), m->nrows_local, m->colidx.get(), pos.get(), s);
    gather_complex_values(m->nnz, pos.get(), m->val.get(), sorted.get(), s);
    SPL_HIP(hipStreamSynchronize(s));
    m->val = std::move(sorted);
  }
  SPL_HIP(hipStreamSynchronize(s));
}

// the column-major image of a whole handle on the device: dcp[ncols + 1], dri[nnz], dv[nnz * vw]
void csc_image(const Matrix *m, int64_t *dcp, int *dri, double *dv, hipStream_t s) {
  if (m->vw == 1) {
    transpose_compressed(m->rowptr.get(), m->colidx.get(), m->val.get(), m->nrows_local, m->ncols, m->nnz, dcp, dri, dv, s);
  } else {
    DBuf<double> pos((size_t)m->nnz), perm((size_t)m->nnz);
    fill_positions(m->nnz, pos.get(), s);
    transpose_compressed(m->rowptr.get(), m->colidx.get(), pos.get(), m->nrows_local, m->ncols, m->nnz, dcp, dri,
                         perm.get(), s);
    gather_complex_values(m->nnz, perm.get(), m->val.get(), dv, s);
    SPL_HIP(hipStreamSynchronize(s));  // perm is released on return
  }
}

}  // namespace

int spl_matrix_create_csr_dev(int64_t nrows, int64_t ncols, int index_width, const void *d_rowptr, const void *d_colidx,
                              const double *d_val, int value_width, void **H) {
  int st = import_arguments(nrows, ncols, 0, index_width, value_width, H);
  if (st != SPL_OK) return st;
  if (!d_rowptr || !aligned_to(d_rowptr, (size_t)index_width) || !aligned_to(d_colidx, (size_t)index_width) ||
      !aligned_to(d_val, sizeof(double)))
    return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    const int dev = current_device();
    hipStream_t s = nullptr;
    ImportedPattern P;
    bool ascending = true;
    int st = import_pattern(index_width, d_rowptr, d_colidx, d_val, value_width, nrows, ncols, false, P, &ascending, s);
    if (st != SPL_OK) return st;
    std::unique_ptr<Matrix> m = make_matrix(dev, nrows, ncols, 0, nrows, value_width);
    m->nnz = P.nnz;
    m->rowptr64 = std::move(P.p64);
    m->colidx = std::move(P.idx);
    m->val.alloc((size_t)P.nnz * (size_t)value_width);
    if (P.nnz)  // values are moved as bits
      SPL_HIP(hipMemcpyAsync(m->val.get(), d_val, (size_t)P.nnz * (size_t)value_width * sizeof(double),
                             hipMemcpyDeviceToDevice, s));
    if (!ascending) sort_rows(m.get(), s);
    return publish(std::move(m), s, H);
  });
}

int spl_matrix_create_csc_dev(int64_t nrows, int64_t ncols, int index_width, const void *d_colptr, const void *d_rowidx,
                              const double *d_val, int value_width, void **H) {
  int st = import_arguments(nrows, ncols, 0, index_width, value_width, H);
  if (st != SPL_OK) return st;
  if (!d_colptr || !aligned_to(d_colptr, (size_t)index_width) || !aligned_to(d_rowidx, (size_t)index_width) ||
      !aligned_to(d_val, sizeof(double)))
    return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    const int dev = current_device();
    hipStream_t s = nullptr;
    ImportedPattern P;
    // rows inside a column in any order, as spl_matrix_create takes them: the transpose orders the row image
    int st = import_pattern(index_width, d_colptr, d_rowidx, d_val, value_width, ncols, nrows, true, P, nullptr, s);
    if (st != SPL_OK) return st;
    DBuf<int> p32((size_t)ncols + 1);
    narrow_i64_to_i32(P.p64.get(), p32.get(), ncols + 1, s);
    std::unique_ptr<Matrix> m = make_matrix(dev, nrows, ncols, 0, nrows, value_width);
    m->nnz = P.nnz;
    m->rowptr64.alloc((size_t)nrows + 1);
    m->colidx.alloc((size_t)P.nnz);
    m->val.alloc((size_t)P.nnz * (size_t)value_width);
    if (value_width == 1) {  // the values go from the caller's array straight to their place in the row image
      transpose_compressed(p32.get(), P.idx.get(), d_val, ncols, nrows, P.nnz, m->rowptr64.get(), m->colidx.get(),
                           m->val.get(), s);
    } else {  // as build_from_csc: the pattern with the entry positions as payload, the pairs gathered along them
      DBuf<double> pos((size_t)P.nnz), perm((size_t)P.nnz);
      fill_positions(P.nnz, pos.get(), s);
      transpose_compressed(p32.get(), P.idx.get(), pos.get(), ncols, nrows, P.nnz, m->rowptr64.get(), m->colidx.get(),
                           perm.get(), s);
      gather_complex_values(P.nnz, perm.get(), d_val, m->val.get(), s);
      SPL_HIP(hipStreamSynchronize(s));
    }
    return publish(std::move(m), s, H);
  });
}

int spl_matrix_compress_dev_wide(int64_t nrows, int64_t ncols, int64_t ntriples, int index_width, const void *d_rows,
                                 const void *d_cols, const double *d_vals, int value_width, void **H, int64_t *bad) {
  int st = import_arguments(nrows, ncols, ntriples, index_width, value_width, H);
  if (st != SPL_OK) return st;
  if (ntriples >= 0x7fffffffLL) return SPL_ERROR_index_overflow;  // the sort key keeps the input position in 32 bits
  if (ntriples > 0 && (!d_rows || !d_cols || !d_vals)) return SPL_ERROR_argument_missing;
  if (!aligned_to(d_rows, (size_t)index_width) || !aligned_to(d_cols, (size_t)index_width) ||
      !aligned_to(d_vals, sizeof(double)))
    return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    const int dev = current_device();
    hipStream_t s = nullptr;
    // as spl_matrix_compress_dev: the row image is the compress of the exchanged triples, and a bounds-only pass in the
    // caller's order first keeps the reference's order of complaints (rows, then columns)
    {
      DBuf<int> none_i;
      DBuf<double> none_v;
      DBuf<int> probe((size_t)ncols + 1);
      int64_t nz = 0, where = -1;
      int st = compress_device_wide(index_width, value_width, nrows, ncols, ntriples, d_rows, d_cols, d_vals, probe.get(),
                                    none_i, none_v, &nz, &where, s, /*check_only=*/true);
      if (st != SPL_OK) { if (bad) *bad = where; return st; }
    }
    std::unique_ptr<Matrix> C = make_matrix(dev, nrows, ncols, 0, nrows, value_width);
    DBuf<int> ptr32((size_t)nrows + 1);
    int64_t where = -1;
    int st = compress_device_wide(index_width, value_width, ncols, nrows, ntriples, d_cols, d_rows, d_vals, ptr32.get(),
                                  C->colidx, C->val, &C->nnz, &where, s, false);
    if (st != SPL_OK) { if (bad) *bad = where; return st; }
    C->rowptr64.alloc((size_t)nrows + 1);
    widen_i32_to_i64(ptr32.get(), C->rowptr64.get(), nrows + 1, s);
    return publish(std::move(C), s, H);
  });
}

// ---- taking a handle apart (csrc/submatrix.hip) ---------------------------------------------------------------------
// C[i, j] = A[r0 + i, c0 + j]: what the signature and the two guards of `subMatrix` (Sparse.hs:704-729) mean.  The
// reference's own body is not reproduced (it slices with an end where a length belongs, keeps the row indices
// unshifted and builds the column pointers from row indices).  On the row image a window is, per result row, the run
// of the source row between two lower bounds.
int spl_matrix_submatrix(void *H, int64_t r0, int64_t c0, int64_t nr, int64_t nc, void **HC) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if (!HC) return SPL_ERROR_argument_missing;
  *HC = nullptr;
  if (r0 < 0 || c0 < 0 || nr < 0 || nc < 0) return SPL_ERROR_n_nonpositive;
  // the reference's two guards, written so that the sums cannot overflow
  if (nr > A->nrows_global || r0 > A->nrows_global - nr) return SPL_ERROR_dimension_mismatch;
  if (nc > A->ncols || c0 > A->ncols - nc) return SPL_ERROR_dimension_mismatch;
  if (!whole(A)) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    hipStream_t s = nullptr;
    std::unique_ptr<Matrix> C = make_matrix(A->device, nr, nc, 0, nr, A->vw);
    submatrix_handle(A, r0, c0, C.get(), s);
    return publish(std::move(C), s, HC);
  });
}

// C[i, j] = A[I[i], J[j]]: rows may repeat and come in any order, columns come in any order and each at most once
int spl_matrix_select(void *H, int64_t nI, const void *d_I, int64_t nJ, const void *d_J, int index_width, void **HC,
                      int64_t *bad) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if (!HC) return SPL_ERROR_argument_missing;
  *HC = nullptr;
  if (nI < 0 || nJ < 0) return SPL_ERROR_n_nonpositive;
  if (nI >= 0x80000000LL || nJ >= 0x80000000LL) return SPL_ERROR_index_overflow;
  if ((index_width != 4 && index_width != 8) || !aligned_to(d_I, (size_t)index_width) ||
      !aligned_to(d_J, (size_t)index_width))
    return SPL_ERROR_argument_missing;
  if ((!d_I && nI != A->nrows_global) || (!d_J && nJ != A->ncols)) return SPL_ERROR_dimension_mismatch;
  if (!whole(A)) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    hipStream_t s = nullptr;
    std::unique_ptr<Matrix> C = make_matrix(A->device, nI, nJ, 0, nI, A->vw);
    bool ascending = true;
    int64_t where = -1;
    const int st = select_handle(A, index_width, d_I, d_J, C.get(), &ascending, &where, s);
    if (st != SPL_OK) {
      if (st == SPL_ERROR_index_out_of_bounds && bad) *bad = where;
      return st;
    }
    if (!ascending && C->nnz > 0) sort_rows(C.get(), s);
    return publish(std::move(C), s, HC);
  });
}

// ---- the entry-wise layer on handles (csrc/entrywise.hip) ------------------------------------------------------------
// `cmap` with the functions the reference itself maps (Sparse.hs:110-125, Data.Complex.Enhanced): the pattern stays,
// stored zeros included.  The result is the operand's block; SPL_MAP_real / _imag of a complex handle are real.
int spl_matrix_map(void *H, int op, const double scalar[2], void **HC) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if (!HC) return SPL_ERROR_argument_missing;
  *HC = nullptr;
  if (op < SPL_MAP_negate || op > SPL_MAP_scale) return SPL_ERROR_argument_missing;
  double sre = 1.0, sim = 0.0;
  if (op == SPL_MAP_scale) {
    if (!scalar) return SPL_ERROR_argument_missing;
    sre = scalar[0];
    sim = scalar[1];
    if (A->vw == 1 && sim != 0.0) return SPL_ERROR_argument_missing;  // complex scalars: spl_matrix_to_complex first
  }
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    hipStream_t s = nullptr;
    const int vw = (op == SPL_MAP_real || op == SPL_MAP_imag) ? 1 : A->vw;
    std::unique_ptr<Matrix> C = make_matrix(A->device, A->nrows_global, A->ncols, A->row0, A->nrows_local, vw);
    map_handle(A, op, sre, sim, C.get(), s);
    return publish(std::move(C), s, HC);
  });
}

// diag(r) A diag(c) without the two SpGEMMs: (r[i] * a) * c[j], a vector that is NULL is not multiplied with
int spl_matrix_scale_rows_cols(void *H, const double *d_r, const double *d_c, void **HC) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if (!HC) return SPL_ERROR_argument_missing;
  *HC = nullptr;
  if (!aligned_to(d_r, sizeof(double)) || !aligned_to(d_c, sizeof(double))) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    hipStream_t s = nullptr;
    std::unique_ptr<Matrix> C = make_matrix(A->device, A->nrows_global, A->ncols, A->row0, A->nrows_local, A->vw);
    scale_rows_cols_handle(A, d_r, d_c, C.get(), s);
    return publish(std::move(C), s, HC);
  });
}

// the reference never prunes (explicit zeros are first-class); this is the pass a user asks for
int spl_matrix_filter(void *H, int keep, const double param[1], void **HC) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if (!HC) return SPL_ERROR_argument_missing;
  *HC = nullptr;
  if (keep != SPL_KEEP_nonzero && keep != SPL_KEEP_abs_above) return SPL_ERROR_argument_missing;
  double tol = 0.0;
  if (keep == SPL_KEEP_abs_above) {
    if (!param || !(param[0] >= 0.0)) return SPL_ERROR_argument_missing;  // negative, or NaN
    tol = param[0];
  }
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    hipStream_t s = nullptr;
    std::unique_ptr<Matrix> C = make_matrix(A->device, A->nrows_global, A->ncols, A->row0, A->nrows_local, A->vw);
    filter_handle(A, keep, tol, C.get(), s);
    return publish(std::move(C), s, HC);
  });
}

// lo <= j - i <= hi with i the global row: tril, triu and the pieces of A = L + D + U
int spl_matrix_band(void *H, int64_t lo, int64_t hi, void **HC) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if (!HC) return SPL_ERROR_argument_missing;
  *HC = nullptr;
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    hipStream_t s = nullptr;
    std::unique_ptr<Matrix> C = make_matrix(A->device, A->nrows_global, A->ncols, A->row0, A->nrows_local, A->vw);
    band_handle(A, lo, hi, C.get(), s);
    return publish(std::move(C), s, HC);
  });
}

int spl_matrix_reduce_dev(void *H, int what, int axis, double *d_out, void *stream) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if ((what != SPL_REDUCE_abs_sum && what != SPL_REDUCE_abs_max) || (axis != 0 && axis != 1))
    return SPL_ERROR_argument_missing;
  if (axis == 0 && !whole(A)) return SPL_ERROR_argument_missing;
  const int64_t n = axis == 1 ? A->nrows_local : A->ncols;
  if (n > 0 && (!d_out || !aligned_to(d_out, sizeof(double)))) return SPL_ERROR_argument_missing;
  if (axis == 0 && what == SPL_REDUCE_abs_sum && A->nnz > 0 && !A->rowptr.get()) return SPL_ERROR_index_overflow;
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    reduce_handle(A, what, axis, d_out, as_stream(stream));
    return SPL_OK;
  });
}

int spl_matrix_norm(void *H, int which, double *result) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if (!result) return SPL_ERROR_argument_missing;
  if (which < SPL_NORM_one || which > SPL_NORM_max) return SPL_ERROR_argument_missing;
  if (!whole(A)) return SPL_ERROR_argument_missing;
  if (which == SPL_NORM_one && A->nnz > 0 && !A->rowptr.get()) return SPL_ERROR_index_overflow;
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    *result = norm_handle(A, which, nullptr);
    return SPL_OK;
  });
}

void spl_matrix_free(void **H) { free_object(H, as_matrix, delete_object<Matrix>); }

int spl_matrix_info(void *H, int64_t info[8]) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  if (!info) return SPL_ERROR_argument_missing;
  info[0] = m->nrows_global;
  info[1] = m->ncols;
  info[2] = m->row0;
  info[3] = m->nrows_local;
  info[4] = m->nnz;
  info[5] = m->device;
  const int kern = spmv_kernel_in_use(m);
  info[6] = kern == 8 ? m->blocked->R : kern == 16 ? m->panel->P : kern == 15 ? -64 : 0;  // -64: sliced-ELL image
  info[7] = kern == 8 ? m->blocked->w : kern == 16 ? m->panel->w : 0;
  return SPL_OK;
}

int spl_matrix_spmv_kernel(void *H) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  return spmv_kernel_in_use(m);
}

int spl_matrix_export_csr(void *H, int64_t *rowptr, int *colidx, double *val) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  if (!rowptr || (m->nnz > 0 && (!colidx || !val))) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    DeviceGuard g(m->device);
    SPL_HIP(hipMemcpy(rowptr, m->rowptr64.get(), ((size_t)m->nrows_local + 1) * sizeof(int64_t),
                      hipMemcpyDeviceToHost));
    if (m->nnz) {
      SPL_HIP(hipMemcpy(colidx, m->colidx.get(), (size_t)m->nnz * sizeof(int), hipMemcpyDeviceToHost));
      SPL_HIP(hipMemcpy(val, m->val.get(), (size_t)m->nnz * (size_t)m->vw * sizeof(double), hipMemcpyDeviceToHost));
    }
    return SPL_OK;
  });
}

int spl_matrix_export_csr_rows(void *H, int64_t row0, int64_t row1, int64_t *rowptr, int64_t capacity, int *colidx,
                               double *val) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  if (m->vw != 1) return SPL_ERROR_argument_missing;
  if (!rowptr || row0 < 0 || row1 < row0 || row1 > m->nrows_local || capacity < 0) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    DeviceGuard g(m->device);
    SPL_HIP(hipMemcpy(rowptr, m->rowptr64.get() + row0, ((size_t)(row1 - row0) + 1) * sizeof(int64_t),
                      hipMemcpyDeviceToHost));
    const int64_t a = rowptr[0], b = rowptr[row1 - row0];
    if (b - a > capacity || (b > a && (!colidx || !val))) return SPL_ERROR_argument_missing;
    if (b > a) {
      SPL_HIP(hipMemcpy(colidx, m->colidx.get() + a, (size_t)(b - a) * sizeof(int), hipMemcpyDeviceToHost));
      SPL_HIP(hipMemcpy(val, m->val.get() + a, (size_t)(b - a) * sizeof(double), hipMemcpyDeviceToHost));
    }
    return SPL_OK;
  });
}

int spl_matrix_export_csc(void *H, int64_t *colptr, int *rowidx, double *val) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  if (m->vw != 1) return SPL_ERROR_argument_missing;  // complex handles: SpMV only
  if (!colptr || (m->nnz > 0 && (!rowidx || !val))) return SPL_ERROR_argument_missing;
  if (!m->rowptr.get()) return SPL_ERROR_index_overflow;
  return guarded([&]() -> int {
    DeviceGuard g(m->device);
    hipStream_t s = nullptr;
    DBuf<int64_t> dcp((size_t)m->ncols + 1);
    DBuf<int> dri((size_t)m->nnz);
    DBuf<double> dv((size_t)m->nnz);
    transpose_compressed(m->rowptr.get(), m->colidx.get(), m->val.get(), m->nrows_local, m->ncols, m->nnz,
                         dcp.get(), dri.get(), dv.get(), s);
    SPL_HIP(hipMemcpy(colptr, dcp.get(), ((size_t)m->ncols + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (m->nnz) {
      SPL_HIP(hipMemcpy(rowidx, dri.get(), (size_t)m->nnz * sizeof(int), hipMemcpyDeviceToHost));
      SPL_HIP(hipMemcpy(val, dv.get(), (size_t)m->nnz * sizeof(double), hipMemcpyDeviceToHost));
    }
    return SPL_OK;
  });
}

namespace {
// the ladder of the two device exports; *m receives the handle
int export_arguments(void *H, int index_width, const void *d_ptr, const void *d_idx, const double *d_val, Matrix **m) {
  *m = as_matrix(H);
  if (!*m) return SPL_ERROR_invalid_handle;
  if (index_width != 4 && index_width != 8) return SPL_ERROR_argument_missing;
  if (!d_ptr || !aligned_to(d_ptr, (size_t)index_width) || !aligned_to(d_idx, (size_t)index_width) ||
      !aligned_to(d_val, sizeof(double)))
    return SPL_ERROR_argument_missing;
  if ((*m)->nnz > 0 && (!d_idx || !d_val)) return SPL_ERROR_argument_missing;
  if (index_width == 4 && (*m)->nnz >= 0x7fffffffLL) return SPL_ERROR_index_overflow;
  return SPL_OK;
}
}  // namespace

int spl_matrix_export_csr_dev(void *H, int index_width, void *d_rowptr, void *d_colidx, double *d_val) {
  Matrix *m = nullptr;
  int st = export_arguments(H, index_width, d_rowptr, d_colidx, d_val, &m);
  if (st != SPL_OK) return st;
  return guarded([&]() -> int {
    DeviceGuard g(m->device);
    hipStream_t s = nullptr;
    const int64_t np = m->nrows_local + 1;
    if (index_width == 8) {
      SPL_HIP(hipMemcpyAsync(d_rowptr, m->rowptr64.get(), (size_t)np * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
      if (m->nnz) widen_i32_to_i64(m->colidx.get(), static_cast<int64_t *>(d_colidx), m->nnz, s);
    } else {
      narrow_i64_to_i32(m->rowptr64.get(), static_cast<int *>(d_rowptr), np, s);
      if (m->nnz)
        SPL_HIP(hipMemcpyAsync(d_colidx, m->colidx.get(), (size_t)m->nnz * sizeof(int), hipMemcpyDeviceToDevice, s));
    }
    if (m->nnz)
      SPL_HIP(hipMemcpyAsync(d_val, m->val.get(), (size_t)m->nnz * (size_t)m->vw * sizeof(double),
                             hipMemcpyDeviceToDevice, s));
    SPL_HIP(hipStreamSynchronize(s));
    return SPL_OK;
  });
}

int spl_matrix_export_csc_dev(void *H, int index_width, void *d_colptr, void *d_rowidx, double *d_val) {
  Matrix *m = nullptr;
  int st = export_arguments(H, index_width, d_colptr, d_rowidx, d_val, &m);
  if (st != SPL_OK) return st;
  if (!m->rowptr.get()) return SPL_ERROR_index_overflow;  // as spl_matrix_export_csc
  return guarded([&]() -> int {
    DeviceGuard g(m->device);
    hipStream_t s = nullptr;
    // the transpose writes what has the caller's width straight into the caller's arrays (the values always); only the
    // array of the other width passes through a temporary and one converting copy.  nnz == 0: only pointers are written.
    if (index_width == 8) {
      DBuf<int> dri((size_t)m->nnz);
      csc_image(m, static_cast<int64_t *>(d_colptr), dri.get(), d_val, s);
      if (m->nnz) widen_i32_to_i64(dri.get(), static_cast<int64_t *>(d_rowidx), m->nnz, s);
    } else {
      DBuf<int64_t> dcp((size_t)m->ncols + 1);
      csc_image(m, dcp.get(), static_cast<int *>(d_rowidx), d_val, s);
      narrow_i64_to_i32(dcp.get(), static_cast<int *>(d_colptr), m->ncols + 1, s);
    }
    SPL_HIP(hipStreamSynchronize(s));  // the temporaries are released on return
    return SPL_OK;
  });
}

int spl_matrix_mulv(void *H, int xlen, const double *x, double *y) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  return guarded([&]() -> int { return host_spmv(m, xlen, x, (int)m->nrows_local, y, 0); });
}

int spl_matrix_gaxpy(void *H, int xlen, const double *x, int ylen, double *y) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  return guarded([&]() -> int { return host_spmv(m, xlen, x, ylen, y, 1); });
}

int spl_matrix_spmv_dev(void *H, const double *d_x, double *d_y, int accumulate, void *stream) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  if ((m->ncols > 0 && !d_x) || (m->nrows_local > 0 && !d_y)) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    DeviceGuard g(m->device);
    return launch_spmv(m, d_x, d_y, accumulate, as_stream(stream));
  });
}

int spl_matrix_set_variant(void *H, int variant) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  if (m->vw != 1) return variant == 0 ? SPL_OK : SPL_ERROR_argument_missing;  // complex: the one native kernel
  if (variant < 0 || variant >= kNumSpmvVariants) return SPL_ERROR_argument_missing;
  if (variant >= 12 && variant <= 14) {
    // timing-only ablations of the CSR-stream kernel (they do NOT compute A x): refuse them unless
    // a profiling session asks explicitly
    const char *ok = getenv("SPL_ALLOW_ABLATION");
    if (!(ok && ok[0] == '1')) return SPL_ERROR_argument_missing;
  }
  if (variant == 8 && !m->blocked) {
    int st = spl_matrix_build_blocked(H, 0, 0, 0);
    if (st != SPL_OK) return st;
  }
  if (variant == 16 && !m->panel) {
    int st = spl_matrix_build_panel(H, 0, 0, 0, 0);
    if (st != SPL_OK) return st;
  }
  if (variant == 15 && !m->sell) {
    int st = guarded([&]() -> int {
      DeviceGuard g(m->device);
      build_sell_image(m, nullptr);
      return SPL_OK;
    });
    if (st != SPL_OK) return st;
  }
  m->variant = variant;
  return SPL_OK;
}

int spl_matrix_build_blocked(void *H, int rows_per_panel, int cols_log2, int unroll) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  if (m->vw != 1) return SPL_ERROR_argument_missing;
  int waves = 16;
  if (rows_per_panel == 0 && cols_log2 == 0) {
    {
      int st = guarded([&]() -> int { DeviceGuard g(m->device); measure_locality(m, nullptr); return SPL_OK; });
      if (st != SPL_OK) return st;
    }
    choose_blocking(m, &rows_per_panel, &cols_log2, &waves);
    if (rows_per_panel == 0) { rows_per_panel = 1024; cols_log2 = 18; waves = 16; }  // explicit request: default shape
  }
  if (const char *ev = getenv("SPL_BLOCKED_LOCKSTEP")) waves = atoi(ev);
  if (waves != 0 && waves != 8 && waves != 4) waves = 16;
  if (rows_per_panel < 1 || rows_per_panel > 20480 || cols_log2 < 4 || cols_log2 > 26 ||
      ((int64_t)rows_per_panel << cols_log2) > 0x7fffffffLL)
    return SPL_ERROR_argument_missing;
  // the lockstep workgroup keeps `waves` panels in one CU's LDS (160 KiB)
  while (waves > 0 && (size_t)waves * (size_t)rows_per_panel * sizeof(double) > 160 * 1024)
    waves = waves == 16 ? 8 : waves == 8 ? 4 : 0;
  if (waves == 0 && (size_t)4 * (size_t)rows_per_panel * sizeof(double) > 160 * 1024)
    return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    DeviceGuard g(m->device);
    build_blocked_image(m, rows_per_panel, cols_log2, nullptr);
    if (unroll == 0) {
      // register pipeline depth: the smallest of {4,8,10,12} chunks that covers the mean segment
      // (longer segments take the un-pipelined tail loop; a deeper pipeline only streams entries
      // of the next segment it cannot use yet — measured at C2: 10 chunks 1.19 ms, 12 chunks 1.22 ms)
      const double seg = (double)m->nnz / (double)(m->blocked->npanels * m->blocked->ncb > 0
                                                       ? m->blocked->npanels * m->blocked->ncb : 1);
      const double want = seg / 64.0;
      unroll = want <= 4 ? 4 : want <= 8 ? 8 : want <= 10 ? 10 : 12;
    }
    m->blocked_unroll = unroll;
    m->blocked->lockstep_waves = waves;
    if (const char *ev = getenv("SPL_BLOCKED_FOLD")) m->blocked->fold = atoi(ev);
    return SPL_OK;
  });
}

int spl_matrix_build_panel(void *H, int rows_per_panel, int cols_log2, int unroll, int form) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  if (m->vw != 1) return SPL_ERROR_argument_missing;
  if (!panel_code_valid(form, unroll)) return SPL_ERROR_argument_missing;
  const bool auto_shape = rows_per_panel == 0 && cols_log2 == 0;
  int nslices = 1;
  if (auto_shape) {
    choose_panels(m, &rows_per_panel, &cols_log2, panel_code_takes_slices(form) ? &nslices : nullptr);
  } else if (form != SPL_PANEL_FORM_DEFAULT && panel_code_takes_slices(form)) {  // explicit shape: slices only on request
    const int f = panel_slices_override();
    if (f >= 1) nslices = f;
  }
  if (rows_per_panel < 1 || rows_per_panel > 20479 || cols_log2 < 4 || cols_log2 > 17)
    return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    DeviceGuard g(m->device);
    const PanelPlan asked = panel_plan_from_code(form, unroll, cols_log2, nslices);
    if (asked.form == PanelForm::Ring &&
        (asked.nl < 1 || asked.slots < 1 || panel_ring_lds_bytes(rows_per_panel, asked.nl, asked.slots) > 160 * 1024))
      return SPL_ERROR_argument_missing;
    build_panel_image(m, rows_per_panel, cols_log2, asked.form != PanelForm::Chunk, nullptr);
    m->panel->plan = choose_panel_plan(m, m->panel, form, unroll, nslices, auto_shape);
    return SPL_OK;
  });
}

int spl_matrix_panel_errors(void *H) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  int out = 0;
  int st = guarded([&]() -> int { DeviceGuard g(m->device); out = panel_ring_errors(m, nullptr); return SPL_OK; });
  return st != SPL_OK ? st : out;
}

int spl_matrix_set_spmv_order(void *H, int order) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  if (order != SPL_ORDER_REFERENCE && order != SPL_ORDER_FREE) return SPL_ERROR_argument_missing;
  m->order_free = order == SPL_ORDER_FREE;
  return SPL_OK;
}

int spl_matrix_set_reserved_cus(void *H, int reserved) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  if (reserved < 0) return SPL_ERROR_argument_missing;
  m->reserved_cus = reserved;
  return SPL_OK;
}

int spl_matrix_optimize(void *H) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  if (m->vw != 1) return SPL_OK;  // complex: the CSR-stream kernel of spmv_z.hip is the one there is
  int R = 0, w = 0, waves = 16;
  {
    int st = guarded([&]() -> int { DeviceGuard g(m->device); measure_locality(m, nullptr); return SPL_OK; });
    if (st != SPL_OK) return st;
  }
  if (panels_beat_stream(m)) return spl_matrix_build_panel(H, 0, 0, 0, 0);
  choose_blocking(m, &R, &w, &waves);
  if (R == 0) {
    // no blocking needed.  Regular rows with column locality (banded, stencil): the sliced-ELL
    // image turns the x gathers into near-coalesced loads; build it when padding stays < 1/8.
    if (m->nnz > 0 && m->new_line_fraction < 0.5 && m->nrows_local >= 64 * 256) {
      return guarded([&]() -> int {
        DeviceGuard g(m->device);
        const int64_t padded = sell_padded_entries(m, nullptr);
        if (padded - m->nnz <= m->nnz / 8) build_sell_image(m, nullptr);
        return SPL_OK;
      });
    }
    return SPL_OK;  // the CSR-stream kernel is already the right one
  }
  // order-free sums allowed (spl_matrix_set_spmv_order): the column-sorted panels send fewer requests
  // to the L2 when a panel is tall enough for lines of x to meet several of its entries
  if (m->order_free && panels_pay(m)) return spl_matrix_build_panel(H, 0, 0, 0, 0);
  return spl_matrix_build_blocked(H, 0, 0, 0);  // 0,0: the same choice, including wavefronts per CU
}

int spl_vector_synthetic_dev(uint64_t seed, int64_t j0, int64_t j1, double *d_x, void *stream) {
  if (j1 < j0) return SPL_ERROR_argument_missing;
  if (j1 > j0 && !d_x) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    (void)current_device();
    generate_vector(seed, j0, j1, d_x, as_stream(stream));
    return SPL_OK;
  });
}

// ---- one-shot operations ------------------------------------------------------------------

int spl_gaxpy(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax, int xlen,
              const double *x, int ylen, double *y) {
  // the reference checks dimensions before touching anything (Sparse.hs:438-445)
  if (nrows >= 0 && ncols >= 0 && (xlen != ncols || ylen != nrows)) return SPL_ERROR_dimension_mismatch;
  return guarded([&]() -> int {
    std::unique_ptr<Matrix> m;
    int st = one_shot_image(nrows, ncols, Ap, Ai, Ax, m);
    return st != SPL_OK ? st : host_spmv(m.get(), xlen, x, ylen, y, 1);
  });
}

int spl_mulv(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax, int xlen,
             const double *x, double *y) {
  if (nrows >= 0 && ncols >= 0 && xlen != ncols) return SPL_ERROR_dimension_mismatch;
  return guarded([&]() -> int {
    std::unique_ptr<Matrix> m;
    int st = one_shot_image(nrows, ncols, Ap, Ai, Ax, m);
    return st != SPL_OK ? st : host_spmv(m.get(), xlen, x, nrows, y, 0);
  });
}

int spl_gaxpy_t(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax, int xlen,
                const double *x, int ylen, double *y) {
  if (nrows >= 0 && ncols >= 0 && (xlen != nrows || ylen != ncols)) return SPL_ERROR_dimension_mismatch;
  int st = check_tuple(nrows, ncols, Ap, Ai, Ax);
  if (st != SPL_OK) return st;
  // the CSC arrays of A are the CSR arrays of A^T: no conversion at all
  void *h = nullptr;
  st = spl_matrix_create_csr(ncols, nrows, 0, ncols, Ap, Ai, Ax, &h);
  if (st != SPL_OK) return st;
  st = spl_matrix_gaxpy(h, xlen, x, ylen, y);
  spl_matrix_free(&h);
  return st;
}

int spl_mulm(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax, int brows, int bcols,
             const double *B, double *C) {
  if (nrows >= 0 && ncols >= 0 && ncols != brows) return SPL_ERROR_dimension_mismatch;  // Sparse.hs:478
  if (bcols < 0) return SPL_ERROR_n_nonpositive;
  if ((int64_t)brows * bcols > 0 && !B) return SPL_ERROR_argument_missing;
  if ((int64_t)nrows * bcols > 0 && !C) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    std::unique_ptr<Matrix> m;
    int st = one_shot_image(nrows, ncols, Ap, Ai, Ax, m);
    if (st != SPL_OK) return st;
    hipStream_t s = nullptr;
    const size_t nb = (size_t)brows * bcols, nc = (size_t)nrows * bcols;
    DBuf<double> dB, dC(nc);
    upload(dB, B, nb, s);
    // the reference runs one axpy_ per column of B (Sparse.hs:482-488); the fused kernel reads A
    // once for all columns and keeps each column's evaluation order
    st = launch_spmm(m.get(), dB.get(), dC.get(), bcols, 0, s);
    if (st == SPL_OK && nc) SPL_HIP(hipMemcpyAsync(C, dC.get(), nc * sizeof(double), hipMemcpyDeviceToHost, s));
    SPL_HIP(hipStreamSynchronize(s));
    return st;
  });
}

int spl_matrix_spmm_dev(void *H, const double *d_B, double *d_C, int k, int accumulate, void *stream) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  if (m->vw != 1) return SPL_ERROR_argument_missing;
  if (k < 0) return SPL_ERROR_n_nonpositive;
  if (k > 0 && ((m->ncols > 0 && !d_B) || (m->nrows_local > 0 && !d_C))) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    DeviceGuard g(m->device);
    return launch_spmm(m, d_B, d_C, k, accumulate, as_stream(stream));
  });
}

int spl_matrix_spmv_many_dev(void *H, int k, const double *d_X, int64_t ldx, double *d_Y, int64_t ldy, int accumulate,
                             void *stream) {
  Matrix *m = as_matrix(H);
  if (!m) return SPL_ERROR_invalid_handle;
  if (k < 0) return SPL_ERROR_n_nonpositive;
  if (k == 0) return SPL_OK;
  if ((m->ncols > 0 && !d_X) || (m->nrows_local > 0 && !d_Y)) return SPL_ERROR_argument_missing;
  const uintptr_t entry = (uintptr_t)(8 * m->vw);  // the kernel loads and stores whole entries
  if ((uintptr_t)d_X % entry != 0 || (uintptr_t)d_Y % entry != 0) return SPL_ERROR_argument_missing;
  if (k > 1 && (ldx < m->ncols || ldy < m->nrows_local)) return SPL_ERROR_dimension_mismatch;
  return guarded([&]() -> int {
    DeviceGuard g(m->device);
    return launch_spmv_many(m, k, d_X, ldx, d_Y, ldy, accumulate, as_stream(stream));
  });
}

// ---- sparse triangular solves on handles (csrc/trisolve.hip) ---------------------------------------------------------
// The analysis keeps its own permuted copy of the triangle and the level tables: H is borrowed for the call.
int spl_trisolve_analyze(void *H, int uplo, int diag, void **T) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if (!T) return SPL_ERROR_argument_missing;
  *T = nullptr;
  if ((uplo != SPL_TRI_lower && uplo != SPL_TRI_upper) || (diag != SPL_DIAG_stored && diag != SPL_DIAG_unit))
    return SPL_ERROR_argument_missing;
  if (A->nrows_global != A->ncols) return SPL_ERROR_dimension_mismatch;
  if (!whole(A) || !A->rowptr.get()) return SPL_ERROR_invalid_matrix;
  return create_object<TriSolver>(A, T, [&](TriSolver **S) { return trisolve_analyze(A, uplo, diag, S); });
}

int spl_trisolve_solve_dev(void *T, int op, int k, const double *d_B, int64_t ldb, double *d_X, int64_t ldx,
                           void *stream) {
  TriSolver *S = as_trisolver(T);
  if (!S) return SPL_ERROR_invalid_handle;
  if (k < 0) return SPL_ERROR_n_nonpositive;
  const ObjectHead &o = head(S);
  if (k == 0 || o.n == 0) return SPL_OK;
  if (op != SPL_OP_n && op != SPL_OP_t && op != SPL_OP_h) return SPL_ERROR_argument_missing;
  if (!d_B || !d_X) return SPL_ERROR_argument_missing;
  const uintptr_t entry = (uintptr_t)(8 * o.vw);  // the kernels load and store whole entries
  if ((uintptr_t)d_B % entry != 0 || (uintptr_t)d_X % entry != 0) return SPL_ERROR_argument_missing;
  if (k > 1 && (ldb < o.n || ldx < o.n)) return SPL_ERROR_dimension_mismatch;
  return guarded([&]() -> int {
    DeviceGuard g(o.device);
    return trisolve_solve(S, op, k, d_B, ldb, d_X, ldx, as_stream(stream));
  });
}

// host arrays, n x k column-major without padding: up, solved in place on the device, down
int spl_trisolve_solve(void *T, int op, int k, const double *B, double *X) {
  TriSolver *S = as_trisolver(T);
  if (!S) return SPL_ERROR_invalid_handle;
  if (k < 0) return SPL_ERROR_n_nonpositive;
  const ObjectHead &o = head(S);
  if (k == 0 || o.n == 0) return SPL_OK;
  if (op != SPL_OP_n && op != SPL_OP_t && op != SPL_OP_h) return SPL_ERROR_argument_missing;
  if (!B || !X) return SPL_ERROR_argument_missing;
  const size_t count = (size_t)o.n * (size_t)k * (size_t)o.vw;
  return with_host_vectors(o.device, count, 1, B, nullptr, 0, X, [&](double *d, hipStream_t s) {
    return trisolve_solve(S, op, k, d, o.n, d, o.n, s);
  });
}

int spl_trisolve_info(void *T, int64_t info[8]) { return info_of(T, as_trisolver, trisolve_info, info); }

void spl_trisolve_free(void **T) { free_object(T, as_trisolver, trisolve_delete); }

// ---- ILU(0) on handles (csrc/ilu0.hip) ---------------------------------------------------------------------------------
// The plan keeps its own device copy of the pattern and the level tables, no values: H is borrowed for the call.
int spl_ilu0_analyze(void *H, void **P) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if (!P) return SPL_ERROR_argument_missing;
  *P = nullptr;
  if (A->nrows_global != A->ncols) return SPL_ERROR_dimension_mismatch;
  if (!whole(A) || !A->rowptr.get()) return SPL_ERROR_invalid_matrix;
  return create_object<IluPlan>(A, P, [&](IluPlan **S) { return ilu0_analyze(A, S); });
}

// F: a new ordinary handle with H's pattern and the L\U values; H any whole handle with the analysed pattern
int spl_ilu0_factor(void *P, void *H, void **F) {
  IluPlan *S = as_ilu_plan(P);
  Matrix *A = as_matrix(H);
  if (!S || !A) return SPL_ERROR_invalid_handle;
  if (!F) return SPL_ERROR_argument_missing;
  *F = nullptr;
  if (!whole(A) || !A->rowptr.get() || A->device != head(S).device) return SPL_ERROR_invalid_matrix;
  return guarded([&]() -> int {
    DeviceGuard g(A->device);
    hipStream_t s = nullptr;
    std::unique_ptr<Matrix> C = make_matrix(A->device, A->nrows_global, A->ncols, 0, A->nrows_local, A->vw);
    const int st = ilu0_factor(S, A, C.get(), s);
    if (st < 0) return st;
    publish(std::move(C), s, F);
    return st;
  });
}

int spl_ilu0_info(void *P, int64_t info[8]) { return info_of(P, as_ilu_plan, ilu0_info, info); }

void spl_ilu0_free(void **P) { free_object(P, as_ilu_plan, ilu0_delete); }

// analyze + factor + free: the one-shot form
int spl_matrix_ilu0(void *H, void **F) {
  if (!as_matrix(H)) return SPL_ERROR_invalid_handle;
  if (!F) return SPL_ERROR_argument_missing;
  *F = nullptr;
  void *plan = nullptr;
  int st = spl_ilu0_analyze(H, &plan);
  if (st < 0) return st;
  st = spl_ilu0_factor(plan, H, F);
  spl_ilu0_free(&plan);
  return st;
}

// ---- the fixed-order inner product, preconditioned CG and BiCGSTAB on handles (csrc/krylov.hip) ------------------------
int spl_vector_dot_dev(int64_t n, int value_width, const double *d_a, const double *d_b, double *d_out, void *stream) {
  if (n < 0) return SPL_ERROR_n_nonpositive;
  if (value_width != 1 && value_width != 2) return SPL_ERROR_argument_missing;
  if (!d_out || (n > 0 && (!d_a || !d_b))) return SPL_ERROR_argument_missing;
  const uintptr_t entry = (uintptr_t)(8 * value_width);  // the kernels load and store whole entries
  if ((uintptr_t)d_a % entry != 0 || (uintptr_t)d_b % entry != 0 || (uintptr_t)d_out % entry != 0)
    return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    return vector_dot(current_device(), n, value_width, d_a, d_b, d_out, as_stream(stream));
  });
}

// A is borrowed: the object keeps the pointer and its own work vectors
int spl_krylov_create(void *A, int method, void **K) {
  Matrix *M = nullptr;
  const int refused = square_whole_matrix(A, K, method == SPL_KRYLOV_cg || method == SPL_KRYLOV_bicgstab, &M);
  if (refused != SPL_OK) return refused;
  return create_object<Krylov>(M, K, [&](Krylov **S) { return krylov_create(M, method, S); });
}

int spl_krylov_set_preconditioner(void *K, void *T1, const double *d_mid, void *T2) {
  return set_preconditioner_of(K, as_krylov, krylov_set_preconditioner, T1, d_mid, T2);
}

int spl_krylov_solve_dev(void *K, const double *d_b, double *d_x, int use_x0, double rtol, double atol, int64_t max_iter,
                         int check_every, int64_t result[4], double *history, void *stream) {
  Krylov *S = as_krylov(K);
  int refused = check_linear_solve(S != nullptr, result != nullptr, rtol, atol, max_iter, check_every, history);
  if (refused != SPL_OK) return refused;
  const ObjectHead &o = head(S);
  if (o.n == 0) {
    empty_linear_result(4, result, history);
    return SPL_OK;
  }
  if ((refused = check_device_vectors(o, d_b, d_x)) != SPL_OK) return refused;
  return guarded([&]() -> int {
    DeviceGuard g(o.device);
    return krylov_solve(S, d_b, d_x, use_x0 ? 1 : 0, rtol, atol, max_iter, check_every, result, history, as_stream(stream));
  });
}

// host vectors of n entries, packed complex: up, solved on the default stream with the default check interval, down
int spl_krylov_solve(void *K, const double *b, double *x, int use_x0, double rtol, double atol, int64_t max_iter,
                     int64_t result[4], double *history) {
  Krylov *S = as_krylov(K);
  const int refused = check_linear_solve(S != nullptr, result != nullptr, rtol, atol, max_iter, 0, history);
  if (refused != SPL_OK) return refused;
  const ObjectHead &o = head(S);
  if (o.n == 0) {
    empty_linear_result(4, result, history);
    return SPL_OK;
  }
  if (!b || !x) return SPL_ERROR_argument_missing;
  const size_t count = (size_t)o.n * (size_t)o.vw;
  return with_host_vectors(o.device, count, 2, b, use_x0 ? x : nullptr, 1, x, [&](double *d, hipStream_t s) {
    return krylov_solve(S, d, d + count, use_x0 ? 1 : 0, rtol, atol, max_iter, 0, result, history, s);
  });
}

int spl_krylov_info(void *K, int64_t info[8]) { return info_of(K, as_krylov, krylov_info, info); }

void spl_krylov_free(void **K) { free_object(K, as_krylov, krylov_delete); }

// ---- multicolour ordering on handles (csrc/coloring.hip) --------------------------------------------------------------
// H is borrowed for the call; d_colors and d_perm are the caller's device arrays, *offsets a malloc()'d host array
int spl_matrix_color(void *H, int order, uint64_t seed, int *d_colors, int *d_perm, int64_t **offsets, int64_t info[8]) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if (offsets) *offsets = nullptr;
  if (!d_colors || !info) return SPL_ERROR_argument_missing;
  if (order != SPL_COLOR_hash) return SPL_ERROR_argument_missing;
  if ((uintptr_t)d_colors % sizeof(int) != 0 || (uintptr_t)d_perm % sizeof(int) != 0) return SPL_ERROR_argument_missing;
  if (A->nrows_global != A->ncols) return SPL_ERROR_dimension_mismatch;
  if (!whole(A) || A->nnz >= (int64_t)0x7fffffff || (A->nrows_local > 0 && !A->rowptr.get())) return SPL_ERROR_invalid_matrix;
  return guarded([&]() -> int {
    (void)current_device();
    DeviceGuard g(A->device);
    return color_handle(A, seed, d_colors, d_perm, offsets, info);
  });
}

int spl_vector_permute_dev(int64_t n, int value_width, const int *d_perm, int inverse, const double *d_in, double *d_out,
                           void *stream) {
  if (n < 0) return SPL_ERROR_n_nonpositive;
  if (value_width != 1 && value_width != 2) return SPL_ERROR_argument_missing;
  if (n > 0 && (!d_perm || !d_in || !d_out || d_in == d_out)) return SPL_ERROR_argument_missing;
  const uintptr_t entry = (uintptr_t)(8 * value_width);  // the kernel loads and stores whole entries
  if ((uintptr_t)d_perm % sizeof(int) != 0 || (uintptr_t)d_in % entry != 0 || (uintptr_t)d_out % entry != 0)
    return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    (void)current_device();
    if (n > 0) vector_permute(n, value_width, d_perm, inverse, d_in, d_out, as_stream(stream));
    return SPL_OK;
  });
}

// ---- aggregation AMG on handles (csrc/amg.hip) ---------------------------------------------------------------------------
// H is borrowed for the call; d_agg and d_roots are the caller's device arrays
int spl_matrix_aggregate(void *H, uint64_t seed, int *d_agg, int *d_roots, int64_t info[8]) {
  Matrix *A = as_matrix(H);
  if (!A) return SPL_ERROR_invalid_handle;
  if (!d_agg || !info) return SPL_ERROR_argument_missing;
  if ((uintptr_t)d_agg % sizeof(int) != 0 || (uintptr_t)d_roots % sizeof(int) != 0) return SPL_ERROR_argument_missing;
  if (A->nrows_global != A->ncols) return SPL_ERROR_dimension_mismatch;
  if (!whole(A) || A->nnz >= (int64_t)0x7fffffff || (A->nrows_local > 0 && !A->rowptr.get())) return SPL_ERROR_invalid_matrix;
  return guarded([&]() -> int {
    (void)current_device();
    DeviceGuard g(A->device);
    return aggregate_handle(A, seed, d_agg, d_roots, info);
  });
}

// A is borrowed: the object keeps the pointer; every other level, the weights and the work vectors are its own
int spl_amg_create(void *A, const int64_t opt[8], void **M) {
  Matrix *H = as_matrix(A);
  if (!H) return SPL_ERROR_invalid_handle;
  if (!M) return SPL_ERROR_argument_missing;
  *M = nullptr;
  int64_t o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (opt) memcpy(o, opt, sizeof(o));
  if (o[1] == 0) o[1] = 1;
  if (o[2] == 0) o[2] = 256;
  if (o[3] == 0) o[3] = 16;
  if (o[4] == 0) o[4] = 4;
  if (o[1] < 1 || o[1] > 4 || o[2] < 0 || o[3] < 1 || o[3] > 64 || o[4] < 1 || o[4] > 64 || (o[5] & ~(int64_t)1) != 0 ||
      o[6] != 0 || o[7] != 0)
    return SPL_ERROR_argument_missing;
  if (H->nrows_global != H->ncols) return SPL_ERROR_dimension_mismatch;
  if (!whole(H) || H->nnz >= (int64_t)0x7fffffff || (H->nrows_local > 0 && !H->rowptr.get())) return SPL_ERROR_invalid_matrix;
  return create_object<Amg>(H, M, [&](Amg **S) { return amg_create(H, o, S); });
}

int spl_amg_info(void *M, int64_t info[8]) { return info_of(M, as_amg, amg_info, info); }

// the handles and the weights are lent: they live as long as M does and are not the caller's to free
int spl_amg_level(void *M, int level, void **HA, void **HP, void **HR, const double **d_w, int64_t dims[2]) {
  Amg *S = as_amg(M);
  if (!S) return SPL_ERROR_invalid_handle;
  int64_t info[8];
  amg_info(S, info);
  if (level < 0 || level >= info[1]) return SPL_ERROR_argument_missing;
  amg_level(S, level, HA, HP, HR, d_w, dims);
  return SPL_OK;
}

int spl_amg_apply_dev(void *M, const double *d_b, double *d_x, void *stream) {
  Amg *S = as_amg(M);
  if (!S) return SPL_ERROR_invalid_handle;
  const ObjectHead &o = head(S);
  if (o.n == 0) return SPL_OK;
  const int refused = check_device_vectors(o, d_b, d_x);
  if (refused != SPL_OK) return refused;
  return guarded([&]() -> int {
    DeviceGuard g(o.device);
    return amg_apply(S, d_b, d_x, as_stream(stream), nullptr);
  });
}

// host vectors of n entries, packed complex: up, one cycle on the default stream, down
int spl_amg_apply(void *M, const double *b, double *x) {
  Amg *S = as_amg(M);
  if (!S) return SPL_ERROR_invalid_handle;
  const ObjectHead &o = head(S);
  if (o.n == 0) return SPL_OK;
  if (!b || !x) return SPL_ERROR_argument_missing;
  const size_t count = (size_t)o.n * (size_t)o.vw;
  return with_host_vectors(o.device, count, 2, b, nullptr, 1, x, [&](double *d, hipStream_t s) {
    return amg_apply(S, d, d + count, s, nullptr);
  });
}

void spl_amg_free(void **M) { free_object(M, as_amg, amg_delete); }

// M is borrowed and may serve several solvers; NULL takes the preconditioner away
int spl_krylov_set_preconditioner_amg(void *K, void *M) {
  return set_preconditioner_amg_of(K, as_krylov, krylov_set_preconditioner_amg, M);
}

// ---- restarted GMRES on handles and the fused multi-vector inner product (csrc/gmres.hip) -------------------------------
int spl_vector_dots_dev(int64_t n, int value_width, int k, const double *d_V, int64_t ldv, const double *d_w, double *d_out,
                        void *stream) {
  if (n < 0) return SPL_ERROR_n_nonpositive;
  if (value_width != 1 && value_width != 2) return SPL_ERROR_argument_missing;
  if (k < 1 || k > 128 || ldv < n) return SPL_ERROR_argument_missing;
  if (!d_out || (n > 0 && (!d_V || !d_w))) return SPL_ERROR_argument_missing;
  const uintptr_t entry = (uintptr_t)(8 * value_width);  // the kernels load and store whole entries
  if ((uintptr_t)d_V % entry != 0 || (uintptr_t)d_w % entry != 0 || (uintptr_t)d_out % entry != 0)
    return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    return vector_dots(current_device(), n, value_width, k, d_V, ldv, d_w, d_out, as_stream(stream));
  });
}

// ---- a block of inner products in one pass (csrc/gram.hip) ---------------------------------------------------------------
int spl_vector_gram_dev(int64_t n, int value_width, int k, int l, const double *d_V, int64_t ldv, const double *d_W,
                        int64_t ldw, double *d_G, int64_t ldg, int upper, void *stream) {
  if (n < 0) return SPL_ERROR_n_nonpositive;
  if (value_width != 1 && value_width != 2) return SPL_ERROR_argument_missing;
  if (k < 1 || k > 128 || l < 1 || l > 128 || (upper != 0 && upper != 1) || ldv < n || ldw < n || ldg < k)
    return SPL_ERROR_argument_missing;
  if (!d_G || (n > 0 && (!d_V || !d_W))) return SPL_ERROR_argument_missing;
  const uintptr_t entry = (uintptr_t)(8 * value_width);  // the kernels load and store whole entries
  if ((uintptr_t)d_V % entry != 0 || (uintptr_t)d_W % entry != 0 || (uintptr_t)d_G % entry != 0)
    return SPL_ERROR_argument_missing;
  if (n > 0) {  // G beside the blocks, not inside them
    const uintptr_t g0 = (uintptr_t)d_G, g1 = g0 + ((uintptr_t)(l - 1) * (uintptr_t)ldg + (uintptr_t)k) * entry;
    const uintptr_t v0 = (uintptr_t)d_V, v1 = v0 + ((uintptr_t)(k - 1) * (uintptr_t)ldv + (uintptr_t)n) * entry;
    const uintptr_t w0 = (uintptr_t)d_W, w1 = w0 + ((uintptr_t)(l - 1) * (uintptr_t)ldw + (uintptr_t)n) * entry;
    if ((g0 < v1 && v0 < g1) || (g0 < w1 && w0 < g1)) return SPL_ERROR_argument_missing;
  }
  return guarded([&]() -> int {
    return vector_gram(current_device(), n, value_width, k, l, d_V, ldv, d_W, ldw, d_G, ldg, upper, as_stream(stream));
  });
}

// A is borrowed: the object keeps the pointer, its restart + 3 vectors and its tables
int spl_gmres_create(void *A, int restart, void **G) {
  Matrix *M = nullptr;
  const int refused = square_whole_matrix(A, G, restart >= 1 && restart <= 128, &M);
  if (refused != SPL_OK) return refused;
  return create_object<Gmres>(M, G, [&](Gmres **S) { return gmres_create(M, restart, S); });
}

int spl_gmres_set_preconditioner(void *G, void *T1, const double *d_mid, void *T2) {
  return set_preconditioner_of(G, as_gmres, gmres_set_preconditioner, T1, d_mid, T2);
}

// M is borrowed and may serve several solvers; NULL takes the preconditioner away
int spl_gmres_set_preconditioner_amg(void *G, void *M) {
  return set_preconditioner_amg_of(G, as_gmres, gmres_set_preconditioner_amg, M);
}

int spl_gmres_solve_dev(void *G, const double *d_b, double *d_x, int use_x0, double rtol, double atol, int64_t max_iter,
                        int check_every, int64_t result[6], double *history, double residual[2], void *stream) {
  Gmres *S = as_gmres(G);
  int refused = check_linear_solve(S != nullptr, result && residual, rtol, atol, max_iter, check_every, history);
  if (refused != SPL_OK) return refused;
  const ObjectHead &o = head(S);
  if (o.n == 0) {
    empty_linear_result(6, result, history);
    residual[0] = residual[1] = 0.0;
    return SPL_OK;
  }
  if ((refused = check_device_vectors(o, d_b, d_x)) != SPL_OK) return refused;
  return guarded([&]() -> int {
    DeviceGuard g(o.device);
    return gmres_solve(S, d_b, d_x, use_x0 ? 1 : 0, rtol, atol, max_iter, check_every, result, history, residual,
                       as_stream(stream));
  });
}

// host vectors of n entries, packed complex: up, solved on the default stream with a look after every cycle, down
int spl_gmres_solve(void *G, const double *b, double *x, int use_x0, double rtol, double atol, int64_t max_iter,
                    int64_t result[6], double *history, double residual[2]) {
  Gmres *S = as_gmres(G);
  const int refused = check_linear_solve(S != nullptr, result && residual, rtol, atol, max_iter, 0, history);
  if (refused != SPL_OK) return refused;
  const ObjectHead &o = head(S);
  if (o.n == 0) {
    empty_linear_result(6, result, history);
    residual[0] = residual[1] = 0.0;
    return SPL_OK;
  }
  if (!b || !x) return SPL_ERROR_argument_missing;
  const size_t count = (size_t)o.n * (size_t)o.vw;
  return with_host_vectors(o.device, count, 2, b, use_x0 ? x : nullptr, 1, x, [&](double *d, hipStream_t s) {
    return gmres_solve(S, d, d + count, use_x0 ? 1 : 0, rtol, atol, max_iter, 0, result, history, residual, s);
  });
}

int spl_gmres_info(void *G, int64_t info[8]) { return info_of(G, as_gmres, gmres_info, info); }

void spl_gmres_free(void **G) { free_object(G, as_gmres, gmres_delete); }

// ---- thick-restart Lanczos on handles and the in-place basis rotation (csrc/eigsh.hip) ----------------------------------
int spl_vector_rotate_dev(int64_t n, int value_width, int m, int k, double *d_V, int64_t ldv, const double *d_Y, int ldy,
                          double *d_out, int64_t ldo, void *stream) {
  return rotate_checked(n, value_width, m, k, d_V, ldv, d_Y, ldy, d_out, ldo, stream, false);
}

// the same with a complex Y (packed pairs) on complex vectors
int spl_vector_rotate_z_dev(int64_t n, int value_width, int m, int k, double *d_V, int64_t ldv, const double *d_Y, int ldy,
                            double *d_out, int64_t ldo, void *stream) {
  return rotate_checked(n, value_width, m, k, d_V, ldv, d_Y, ldy, d_out, ldo, stream, true);
}

// A is borrowed: the object keeps the pointer, its ncv + 2 vectors and its tables
int spl_eigsh_create(void *A, int ncv, void **E) {
  Matrix *M = nullptr;
  const int refused = square_whole_matrix(A, E, ncv >= 2 && ncv <= 128, &M);
  if (refused != SPL_OK) return refused;
  return create_object<Eigsh>(M, E, [&](Eigsh **S) -> int {
    if (!M->rowptr.get() || hermitian_device(M, nullptr) != 1) return SPL_ERROR_invalid_matrix;
    return eigsh_create(M, ncv, S);
  });
}

// K is borrowed; NULL: the operator is A again
int spl_eigsh_set_inverse(void *E, void *K, double sigma, double rtol, double atol, int64_t max_iter) {
  Eigsh *S = as_eigsh(E);
  if (!S) return SPL_ERROR_invalid_handle;
  Krylov *P = nullptr;
  if (K) {
    P = as_krylov(K);
    if (!P) return SPL_ERROR_invalid_handle;
    if (!same_shape(head(P), head(S))) return SPL_ERROR_dimension_mismatch;
    if (max_iter < 0) return SPL_ERROR_n_nonpositive;
    if (!(rtol >= 0.0) || !(atol >= 0.0) || !std::isfinite(sigma)) return SPL_ERROR_argument_missing;  // a NaN too
  }
  eigsh_set_inverse(S, P, sigma, rtol, atol, max_iter);
  return SPL_OK;
}

int spl_eigsh_solve_dev(void *E, int nev, int which, double tol, double atol, int64_t max_restarts, const double *d_v0,
                        double *values, double *d_vectors, int64_t ldx, double *residuals, int64_t result[6],
                        double *history, void *stream) {
  Eigsh *S = as_eigsh(E);
  const int refused = check_eigen_solve(S, eigsh_ncv, 1, SPL_EIGSH_largest_magnitude, 1, nev, which, tol, atol,
                                        max_restarts, values, residuals, result, history);
  if (refused != SPL_OK) return refused;
  const ObjectHead &o = head(S);
  if (!d_v0 || !d_vectors || ldx < o.n) return SPL_ERROR_argument_missing;
  const uintptr_t entry = (uintptr_t)(8 * o.vw);  // the kernels load and store whole entries
  if ((uintptr_t)d_v0 % entry != 0 || (uintptr_t)d_vectors % entry != 0) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    DeviceGuard g(o.device);
    return eigsh_solve(S, nev, which, tol, atol, max_restarts, d_v0, values, d_vectors, ldx, residuals, result, history,
                       as_stream(stream));
  });
}

// host v0 (n entries, packed complex) and vectors (nev columns, ldx entries apart): up, solved on the default stream, down
int spl_eigsh_solve(void *E, int nev, int which, double tol, double atol, int64_t max_restarts, const double *v0,
                    double *values, double *vectors, int64_t ldx, double *residuals, int64_t result[6], double *history) {
  Eigsh *S = as_eigsh(E);
  const int refused = check_eigen_solve(S, eigsh_ncv, 1, SPL_EIGSH_largest_magnitude, 1, nev, which, tol, atol,
                                        max_restarts, values, residuals, result, history);
  if (refused != SPL_OK) return refused;
  const ObjectHead &o = head(S);
  if (!v0 || !vectors || ldx < o.n) return SPL_ERROR_argument_missing;
  return with_host_columns(o, 1, v0, o.n, nev, vectors, ldx, result, [&](double *d, double *d_vectors, hipStream_t s) {
    return eigsh_solve(S, nev, which, tol, atol, max_restarts, d, values, d_vectors, o.n, residuals, result, history, s);
  });
}

int spl_eigsh_info(void *E, int64_t info[8]) { return info_of(E, as_eigsh, eigsh_info, info); }

void spl_eigsh_free(void **E) { free_object(E, as_eigsh, eigsh_delete); }

// ---- LOBPCG on handles (csrc/lobpcg.hip) -----------------------------------------------------------------------------------
// A is borrowed: the object keeps the pointer, its 7 block + 1 vectors and its tables
int spl_lobpcg_create(void *A, int block, void **L) {
  Matrix *M = nullptr;
  const int refused = square_whole_matrix(A, L, block >= 1 && block <= 42, &M);
  if (refused != SPL_OK) return refused;
  return create_object<Lobpcg>(M, L, [&](Lobpcg **S) -> int {
    if (!M->rowptr.get() || hermitian_device(M, nullptr) != 1) return SPL_ERROR_invalid_matrix;
    return lobpcg_create(M, block, S);
  });
}

int spl_lobpcg_set_preconditioner(void *L, void *T1, const double *d_mid, void *T2) {
  return set_preconditioner_of(L, as_lobpcg, lobpcg_set_preconditioner, T1, d_mid, T2);
}

// M is borrowed and may serve several solvers; NULL takes the preconditioner away
int spl_lobpcg_set_preconditioner_amg(void *L, void *M) {
  return set_preconditioner_amg_of(L, as_lobpcg, lobpcg_set_preconditioner_amg, M);
}

// B is borrowed, as A is; NULL: the standard problem again
int spl_lobpcg_set_mass(void *L, void *B) {
  Lobpcg *S = as_lobpcg(L);
  if (!S) return SPL_ERROR_invalid_handle;
  Matrix *M = nullptr;
  if (B) {
    M = as_matrix(B);
    if (!M) return SPL_ERROR_invalid_handle;
    const ObjectHead &o = head(S);
    if (M->nrows_global != o.n || M->ncols != o.n || M->vw != o.vw || M->device != o.device)
      return SPL_ERROR_dimension_mismatch;
    if (!whole(M) || !M->rowptr.get()) return SPL_ERROR_invalid_matrix;
  }
  return guarded([&]() -> int {
    DeviceGuard g(head(S).device);
    if (M && hermitian_device(M, nullptr) != 1) return SPL_ERROR_invalid_matrix;
    lobpcg_set_mass(S, M);
    return SPL_OK;
  });
}

// ---- the paired update of a column and its image under B (csrc/basis_pair.hpp) ------------------------------------------
int spl_vector_update_pair_dev(int64_t n, int value_width, int k, const double *d_V, int64_t ldv, const double *d_BV,
                               int64_t ldbv, const double *d_coef, double *d_w, double *d_bw, double *d_q, void *stream) {
  if (n < 0) return SPL_ERROR_n_nonpositive;
  if (value_width != 1 && value_width != 2) return SPL_ERROR_argument_missing;
  if (k < 1 || k > 128 || ldv < n || ldbv < n) return SPL_ERROR_argument_missing;
  if (!d_coef || (n > 0 && (!d_V || !d_BV || !d_w || !d_bw))) return SPL_ERROR_argument_missing;
  const uintptr_t entry = (uintptr_t)(8 * value_width);  // the kernel loads and stores whole entries
  if ((uintptr_t)d_V % entry != 0 || (uintptr_t)d_BV % entry != 0 || (uintptr_t)d_coef % entry != 0 ||
      (uintptr_t)d_w % entry != 0 || (uintptr_t)d_bw % entry != 0 || (uintptr_t)d_q % sizeof(double) != 0)
    return SPL_ERROR_argument_missing;
  if (n > 0) {  // w and bw beside each other and beside the blocks, not inside them
    const uintptr_t w0 = (uintptr_t)d_w, w1 = w0 + (uintptr_t)n * entry, b0 = (uintptr_t)d_bw, b1 = b0 + (uintptr_t)n * entry;
    const uintptr_t v0 = (uintptr_t)d_V, v1 = v0 + ((uintptr_t)(k - 1) * (uintptr_t)ldv + (uintptr_t)n) * entry;
    const uintptr_t u0 = (uintptr_t)d_BV, u1 = u0 + ((uintptr_t)(k - 1) * (uintptr_t)ldbv + (uintptr_t)n) * entry;
    if ((w0 < b1 && b0 < w1) || (w0 < v1 && v0 < w1) || (w0 < u1 && u0 < w1) || (b0 < v1 && v0 < b1) ||
        (b0 < u1 && u0 < b1))
      return SPL_ERROR_argument_missing;
  }
  return guarded([&]() -> int {
    return vector_update_pair(current_device(), n, value_width, k, d_V, ldv, d_BV, ldbv, d_coef, d_w, d_bw, d_q,
                              as_stream(stream));
  });
}

int spl_lobpcg_solve_dev(void *L, int nev, int which, double tol, double atol, int64_t max_iter, const double *d_X0,
                         int64_t ldx0, double *values, double *d_vectors, int64_t ldx, double *residuals,
                         int64_t result[8], double *history, void *stream) {
  Lobpcg *S = as_lobpcg(L);
  const int refused = check_eigen_solve(S, lobpcg_block, 0, SPL_EIGSH_smallest_algebraic, 0, nev, which, tol, atol,
                                        max_iter, values, residuals, result, history);
  if (refused != SPL_OK) return refused;
  const ObjectHead &o = head(S);
  if (!d_X0 || !d_vectors || ldx0 < o.n || ldx < o.n) return SPL_ERROR_argument_missing;
  const uintptr_t entry = (uintptr_t)(8 * o.vw);  // the kernels load and store whole entries
  if ((uintptr_t)d_X0 % entry != 0 || (uintptr_t)d_vectors % entry != 0) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    DeviceGuard g(o.device);
    return lobpcg_solve(S, nev, which, tol, atol, max_iter, d_X0, ldx0, values, d_vectors, ldx, residuals, result,
                        history, as_stream(stream));
  });
}

// host X0 (block columns, ldx0 entries apart, packed complex) and vectors (nev columns, ldx entries apart): up, solved on
// the default stream, down
int spl_lobpcg_solve(void *L, int nev, int which, double tol, double atol, int64_t max_iter, const double *X0,
                     int64_t ldx0, double *values, double *vectors, int64_t ldx, double *residuals, int64_t result[8],
                     double *history) {
  Lobpcg *S = as_lobpcg(L);
  const int refused = check_eigen_solve(S, lobpcg_block, 0, SPL_EIGSH_smallest_algebraic, 0, nev, which, tol, atol,
                                        max_iter, values, residuals, result, history);
  if (refused != SPL_OK) return refused;
  const ObjectHead &o = head(S);
  if (!X0 || !vectors || ldx0 < o.n || ldx < o.n) return SPL_ERROR_argument_missing;
  return with_host_columns(o, lobpcg_block(S), X0, ldx0, nev, vectors, ldx, result,
                           [&](double *d, double *d_vectors, hipStream_t s) {
                             return lobpcg_solve(S, nev, which, tol, atol, max_iter, d, o.n, values, d_vectors, o.n,
                                                 residuals, result, history, s);
                           });
}

int spl_lobpcg_info(void *L, int64_t info[8]) { return info_of(L, as_lobpcg, lobpcg_info, info); }

void spl_lobpcg_free(void **L) { free_object(L, as_lobpcg, lobpcg_delete); }

// mulM on Complex Double (the reference's SPECIALIZE instance, Sparse.hs:475): one axpy_ per column of B there; here the
// packed-complex image of A and one multi-vector product.  B and C are row-major like spl_mulm's; the kernel wants one
// vector after the other, so both are turned on the device (the call is bounded by its copies over PCIe).
int spl_mulm_z(int nrows, int ncols, const int *Ap, const int *Ai, const double *Az, int brows, int bcols,
               const double *Bz, double *Cz) {
  if (nrows >= 0 && ncols >= 0 && ncols != brows) return SPL_ERROR_dimension_mismatch;  // Sparse.hs:478
  if (bcols < 0) return SPL_ERROR_n_nonpositive;
  if ((int64_t)brows * bcols > 0 && !Bz) return SPL_ERROR_argument_missing;
  if ((int64_t)nrows * bcols > 0 && !Cz) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    std::unique_ptr<Matrix> m;
    int st = build_from_csc(2, nrows, ncols, Ap, Ai, Az, 0, 1, m);
    if (st != SPL_OK) return st;
    hipStream_t s = nullptr;
    finalize_matrix(m.get(), s);
    const size_t nb = (size_t)brows * bcols, nc = (size_t)nrows * bcols;
    DBuf<double> dB, dX(2 * nb), dY(2 * nc), dC(2 * nc);
    upload(dB, Bz, 2 * nb, s);
    st = transpose_dense(brows, bcols, 2, dB.get(), dX.get(), s);
    if (st == SPL_OK) st = launch_spmv_many(m.get(), bcols, dX.get(), brows, dY.get(), nrows, 0, s);
    if (st == SPL_OK) st = transpose_dense(bcols, nrows, 2, dY.get(), dC.get(), s);
    if (st == SPL_OK && nc) SPL_HIP(hipMemcpyAsync(Cz, dC.get(), 2 * nc * sizeof(double), hipMemcpyDeviceToHost, s));
    SPL_HIP(hipStreamSynchronize(s));
    return st;
  });
}

int spl_transpose(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax, int *Tp, int *Ti,
                  double *Tx) {
  int st = check_tuple(nrows, ncols, Ap, Ai, Ax);
  if (st != SPL_OK) return st;
  if (!Tp) return SPL_ERROR_argument_missing;
  const int64_t nnz = Ap[ncols];
  if (nnz > 0 && (!Ti || !Tx)) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    (void)current_device();
    hipStream_t s = nullptr;
    DeviceCsc A;
    DBuf<int> dTi((size_t)nnz), dTp((size_t)nrows + 1);
    DBuf<double> dTx((size_t)nnz);
    DBuf<int64_t> dTp64((size_t)nrows + 1);
    int v = upload_validated(nrows, ncols, Ap, Ai, Ax, 1, A, s);
    if (v != SPL_OK) return v;
    transpose_compressed(A.p.get(), A.i.get(), A.x.get(), ncols, nrows, nnz, dTp64.get(), dTi.get(), dTx.get(), s);
    narrow_i64_to_i32(dTp64.get(), dTp.get(), (int64_t)nrows + 1, s);
    SPL_HIP(hipMemcpyAsync(Tp, dTp.get(), ((size_t)nrows + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
    if (nnz) {
      SPL_HIP(hipMemcpyAsync(Ti, dTi.get(), (size_t)nnz * sizeof(int), hipMemcpyDeviceToHost, s));
      SPL_HIP(hipMemcpyAsync(Tx, dTx.get(), (size_t)nnz * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    SPL_HIP(hipStreamSynchronize(s));
    return SPL_OK;
  });
}

// ---- assembly / SpGEMM one-shots ------------------------------------------------------------

int spl_spgemm(int nrowsA, int ncolsA, const int *Ap, const int *Ai, const double *Ax, int nrowsB,
               int ncolsB, const int *Bp, const int *Bi, const double *Bx, int *nrowsC, int *ncolsC,
               int **Cp, int **Ci, double **Cx) {
  if (!nrowsC || !ncolsC || !Cp || !Ci || !Cx) return SPL_ERROR_argument_missing;
  *Cp = nullptr; *Ci = nullptr; *Cx = nullptr;
  if (nrowsA >= 0 && ncolsA >= 0 && nrowsB >= 0 && ncolsB >= 0 && ncolsA != nrowsB)
    return SPL_ERROR_dimension_mismatch;  // Sparse.hs:694
  return binary_one_shot(1, {nrowsA, ncolsA, Ap, Ai, Ax}, {nrowsB, ncolsB, Bp, Bi, Bx}, nrowsA, ncolsB, nrowsC, ncolsC,
                         Cp, Ci, Cx, [&](DeviceCsc &A, DeviceCsc &B, DeviceResult &C, hipStream_t s) {
                           spgemm_device(nrowsA, ncolsA, A.p.get(), A.i.get(), A.x.get(), ncolsB, B.p.get(), B.i.get(),
                                         B.x.get(), C.p, C.i, C.x, &C.nnz, nullptr, s);
                           return SPL_OK;
                         });
}

// hcat / vcat / fromBlocks / fromBlocksDiag (Sparse.hs:500-595): nblocks CSC blocks placed at (row_off, col_off)
// of an nrowsC x ncolsC result; see include/sparse_linear_hip.h
int spl_assemble_blocks(int nblocks, const int *nrows, const int *ncols, const int *const *Ap, const int *const *Ai,
                        const double *const *Ax, int value_width, const int *row_off, const int *col_off, int nrowsC,
                        int ncolsC, int **Cp, int **Ci, double **Cx) {
  if (!Cp || !Ci || !Cx) return SPL_ERROR_argument_missing;
  *Cp = nullptr; *Ci = nullptr; *Cx = nullptr;
  if (nblocks < 0 || nrowsC < 0 || ncolsC < 0 || (value_width != 1 && value_width != 2)) return SPL_ERROR_argument_missing;
  if (nblocks > 0 && (!nrows || !ncols || !Ap || !Ai || !Ax || !row_off || !col_off)) return SPL_ERROR_argument_missing;
  for (int b = 0; b < nblocks; ++b) {
    if (nrows[b] < 0 || ncols[b] < 0 || row_off[b] < 0 || col_off[b] < 0 || (int64_t)row_off[b] + nrows[b] > nrowsC ||
        (int64_t)col_off[b] + ncols[b] > ncolsC)
      return SPL_ERROR_dimension_mismatch;
    if (!Ap[b]) return SPL_ERROR_argument_missing;
  }
  return guarded([&]() -> int {
    const int dev = current_device();
    hipStream_t s = nullptr;
    // the images of the blocks' transposes, placed with rows and columns exchanged: that is the transpose of the result,
    // whose row image is the result's CSC fields
    std::vector<std::unique_ptr<Matrix>> image((size_t)nblocks);
    std::vector<const Matrix *> blk((size_t)nblocks);
    std::vector<int64_t> roff((size_t)nblocks), coff((size_t)nblocks);
    int64_t nnzC = 0;
    for (int b = 0; b < nblocks; ++b) {
      const int64_t nz = Ap[b][ncols[b]];
      if (nz < 0 || (nz > 0 && (!Ai[b] || !Ax[b]))) return SPL_ERROR_argument_missing;
      DeviceCsc d;
      int st = upload_validated(nrows[b], ncols[b], Ap[b], Ai[b], Ax[b], value_width, d, s);
      if (st != SPL_OK) return st;
      image[(size_t)b] = transposed_image(dev, nrows[b], ncols[b], value_width, d, s);
      blk[(size_t)b] = image[(size_t)b].get();
      roff[(size_t)b] = col_off[b];
      coff[(size_t)b] = row_off[b];
      nnzC += nz;
    }
    std::vector<int> cut, lptr, list;
    int st = blocks_table(nblocks, blk.data(), roff.data(), coff.data(), ncolsC, nrowsC, cut, lptr, list);
    if (st != SPL_OK) return st;
    if (nnzC >= 0x7fffffffLL) return SPL_ERROR_index_overflow;
    std::unique_ptr<Matrix> C = make_matrix(dev, ncolsC, nrowsC, 0, ncolsC, value_width);
    assemble_handles(nblocks, blk.data(), roff.data(), coff.data(), cut, lptr, list, C.get(), s);
    return download_result(ncolsC, C->nnz, value_width, C->rowptr64.get(), C->colidx.get(), C->val.get(), Cp, Ci, Cx, s);
  });
}

int spl_lin(double alpha, int nrowsA, int ncolsA, const int *Ap, const int *Ai, const double *Ax,
            double beta, int nrowsB, int ncolsB, const int *Bp, const int *Bi, const double *Bx,
            int *nrowsC, int *ncolsC, int **Cp, int **Ci, double **Cx) {
  if (!nrowsC || !ncolsC || !Cp || !Ci || !Cx) return SPL_ERROR_argument_missing;
  *Cp = nullptr; *Ci = nullptr; *Cx = nullptr;
  if (nrowsA >= 0 && ncolsA >= 0 && nrowsB >= 0 && ncolsB >= 0 && (nrowsA != nrowsB || ncolsA != ncolsB))
    return SPL_ERROR_dimension_mismatch;  // Sparse.hs:408-409
  return binary_one_shot(1, {nrowsA, ncolsA, Ap, Ai, Ax}, {nrowsB, ncolsB, Bp, Bi, Bx}, nrowsA, ncolsA, nrowsC, ncolsC,
                         Cp, Ci, Cx, [&](DeviceCsc &A, DeviceCsc &B, DeviceResult &C, hipStream_t s) {
                           lin_device(alpha, A.p.get(), A.i.get(), A.x.get(), beta, B.p.get(), B.i.get(), B.x.get(),
                                      ncolsA, C.p, C.i, C.x, &C.nnz, s);
                           return SPL_OK;
                         });
}

int spl_spgemm_z(int nrowsA, int ncolsA, const int *Ap, const int *Ai, const double *Az, int nrowsB, int ncolsB,
                 const int *Bp, const int *Bi, const double *Bz, int *nrowsC, int *ncolsC, int **Cp, int **Ci,
                 double **Cz) {
  if (!nrowsC || !ncolsC || !Cp || !Ci || !Cz) return SPL_ERROR_argument_missing;
  *Cp = nullptr; *Ci = nullptr; *Cz = nullptr;
  if (nrowsA >= 0 && ncolsA >= 0 && nrowsB >= 0 && ncolsB >= 0 && ncolsA != nrowsB)
    return SPL_ERROR_dimension_mismatch;  // Sparse.hs:694
  return binary_one_shot(2, {nrowsA, ncolsA, Ap, Ai, Az}, {nrowsB, ncolsB, Bp, Bi, Bz}, nrowsA, ncolsB, nrowsC, ncolsC,
                         Cp, Ci, Cz, [&](DeviceCsc &A, DeviceCsc &B, DeviceResult &C, hipStream_t s) {
                           spgemm_device_z(nrowsA, ncolsA, A.p.get(), A.i.get(), A.x.get(), ncolsB, B.p.get(),
                                           B.i.get(), B.x.get(), C.p, C.i, C.x, &C.nnz, nullptr, s);
                           return SPL_OK;
                         });
}

int spl_lin_z(const double alpha[2], int nrowsA, int ncolsA, const int *Ap, const int *Ai, const double *Az,
              const double beta[2], int nrowsB, int ncolsB, const int *Bp, const int *Bi, const double *Bz,
              int *nrowsC, int *ncolsC, int **Cp, int **Ci, double **Cz) {
  if (!nrowsC || !ncolsC || !Cp || !Ci || !Cz || !alpha || !beta) return SPL_ERROR_argument_missing;
  *Cp = nullptr; *Ci = nullptr; *Cz = nullptr;
  if (nrowsA >= 0 && ncolsA >= 0 && nrowsB >= 0 && ncolsB >= 0 && (nrowsA != nrowsB || ncolsA != ncolsB))
    return SPL_ERROR_dimension_mismatch;  // Sparse.hs:408-409
  return binary_one_shot(2, {nrowsA, ncolsA, Ap, Ai, Az}, {nrowsB, ncolsB, Bp, Bi, Bz}, nrowsA, ncolsA, nrowsC, ncolsC,
                         Cp, Ci, Cz, [&](DeviceCsc &A, DeviceCsc &B, DeviceResult &C, hipStream_t s) {
                           lin_device_z(alpha, A.p.get(), A.i.get(), A.x.get(), beta, B.p.get(), B.i.get(), B.x.get(),
                                        ncolsA, C.p, C.i, C.x, &C.nnz, s);
                           return SPL_OK;
                         });
}

int spl_kronecker(int nrowsA, int ncolsA, const int *Ap, const int *Ai, const double *Ax, int nrowsB,
                  int ncolsB, const int *Bp, const int *Bi, const double *Bx, int *nrowsC, int *ncolsC,
                  int **Cp, int **Ci, double **Cx) {
  if (!nrowsC || !ncolsC || !Cp || !Ci || !Cx) return SPL_ERROR_argument_missing;
  *Cp = nullptr; *Ci = nullptr; *Cx = nullptr;
  if (nrowsA < 0 || ncolsA < 0 || nrowsB < 0 || ncolsB < 0) return SPL_ERROR_n_nonpositive;
  if ((int64_t)nrowsA * nrowsB >= 0x7fffffffLL || (int64_t)ncolsA * ncolsB >= 0x7fffffffLL)
    return SPL_ERROR_index_overflow;  // the seam is int32 (Foreign.hs:24-28)
  return binary_one_shot(1, {nrowsA, ncolsA, Ap, Ai, Ax}, {nrowsB, ncolsB, Bp, Bi, Bx}, (int64_t)nrowsA * nrowsB,
                         (int64_t)ncolsA * ncolsB, nrowsC, ncolsC, Cp, Ci, Cx,
                         [&](DeviceCsc &A, DeviceCsc &B, DeviceResult &C, hipStream_t s) -> int {
                           if (A.nnz * B.nnz >= 0x7fffffffLL) return SPL_ERROR_index_overflow;
                           // (A (x) B)^T = A^T (x) B^T: the row image of the result's transpose is its CSC fields
                           const int dev = current_device();
                           const int64_t nr = (int64_t)nrowsA * nrowsB, nc = (int64_t)ncolsA * ncolsB;
                           std::unique_ptr<Matrix> At = transposed_image(dev, nrowsA, ncolsA, 1, A, s),
                                                   Bt = transposed_image(dev, nrowsB, ncolsB, 1, B, s),
                                                   Ct = make_matrix(dev, nc, nr, 0, nc);
                           kronecker_handles(At.get(), Bt.get(), Ct.get(), s);
                           C.p = std::move(Ct->rowptr64);
                           C.i = std::move(Ct->colidx);
                           C.x = std::move(Ct->val);
                           C.nnz = Ct->nnz;
                           return SPL_OK;
                         });
}

int spl_take_diag(int nrows, int ncols, const int *Ap, const int *Ai, const double *Ax, double *d) {
  if (nrows < 0 || ncols < 0) return SPL_ERROR_n_nonpositive;
  const int n = nrows < ncols ? nrows : ncols;
  if (n > 0 && !d) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    const int dev = current_device();
    hipStream_t s = nullptr;
    DeviceCsc A;
    int st = upload_csc(nrows, ncols, Ap, Ai, Ax, 1, A, s);
    if (st != SPL_OK) return st;
    if (n == 0) return SPL_OK;
    DBuf<double> dd((size_t)n);
    std::unique_ptr<Matrix> At = transposed_image(dev, nrows, ncols, 1, A, s);  // the diagonal is its own transpose
    take_diag_handle(At.get(), n, dd.get(), s);
    SPL_HIP(hipMemcpyAsync(d, dd.get(), (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    SPL_HIP(hipStreamSynchronize(s));
    SPL_HIP(hipGetLastError());
    return SPL_OK;
  });
}

int spl_compress(int nrows, int ncols, int64_t nnz, const int *rows, const int *cols, const double *vals,
                 int *Ap, int **Ai, double **Ax, int64_t *bad) {
  if (!Ap || !Ai || !Ax) return SPL_ERROR_argument_missing;
  *Ai = nullptr; *Ax = nullptr;
  if (nrows < 0 || ncols < 0 || nnz < 0) return SPL_ERROR_n_nonpositive;
  if (nnz >= 0x7fffffffLL) return SPL_ERROR_index_overflow;
  if (nnz > 0 && (!rows || !cols || !vals)) return SPL_ERROR_argument_missing;
  return guarded([&]() -> int {
    (void)current_device();
    hipStream_t s = nullptr;
    DBuf<int> dr, dc, dptr((size_t)ncols + 1), oidx;
    DBuf<double> dv, oval;
    upload(dr, rows, (size_t)nnz, s);
    upload(dc, cols, (size_t)nnz, s);
    upload(dv, vals, (size_t)nnz, s);
    int64_t nz = 0;
    int st = compress_device(nrows, ncols, nnz, dr.get(), dc.get(), dv.get(), dptr.get(), oidx, oval, &nz,
                             bad, s);
    if (st != SPL_OK) return st;
    // Ap is the caller's (32-bit pointers straight from the kernel); the entries are malloc()'d like download_result's
    HostArray<int> hi = host_alloc<int>((size_t)(nz ? nz : 1));
    HostArray<double> hx = host_alloc<double>((size_t)(nz ? nz : 1));
    if (!hi || !hx) return SPL_ERROR_out_of_memory;
    SPL_HIP(hipMemcpyAsync(Ap, dptr.get(), ((size_t)ncols + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
    if (nz) {
      SPL_HIP(hipMemcpyAsync(hi.get(), oidx.get(), (size_t)nz * sizeof(int), hipMemcpyDeviceToHost, s));
      SPL_HIP(hipMemcpyAsync(hx.get(), oval.get(), (size_t)nz * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    SPL_HIP(hipStreamSynchronize(s));
    *Ai = hi.release();
    *Ax = hx.release();
    return SPL_OK;
  });
}

}  // extern "C"

// lu_from_handle.hip — what the LU calls on device-resident matrix handles need on the device
// (spl_umfpack_{di,zi}_{symbolic,numeric}_dev, include/umfpack_hip.h; the entry points are in umfpack.hip and
// umfpack_zi.hip): the exact pattern compare, the copy of a handle's rows image and, for complex handles, the
// symmetry test, the diagonal pass and the real 2n x 2n embedding — the streaming work umfpack_zi_numeric does on the
// host and sends over PCIe.  Every kernel streams the rows image (Matrix::rowptr, colidx, val) once and is bound by
// memory bandwidth.
//
// The kernels that need the row of an entry work on tiles of kTileRows rows: the entries of a tile are one contiguous
// range of colidx / val, swept by the workgroup with coalesced loads (16 bytes of value per lane); the tile's row
// pointers are staged in LDS once and an entry finds its row by bisection there (8 steps, no global traffic).
#include <cmath>
#include <cstring>

#include "umfpack_impl.hpp"

namespace spl {

namespace {

constexpr int kTileRows = 256;  // rows per workgroup (= threads): 1 KiB of row pointers in LDS

// the tile's row pointers into LDS; returns the number of rows of the tile
__device__ inline int stage_row_pointers(const int *__restrict__ rowptr, int64_t n, int64_t r0, int *ptr_lds) {
  const int rows = (int)(n - r0 < kTileRows ? n - r0 : kTileRows);
  for (int t = threadIdx.x; t <= rows; t += blockDim.x) ptr_lds[t] = rowptr[r0 + t];
  __syncthreads();
  return rows;
}

// local row of entry p: the last t in [0, rows) with ptr_lds[t] <= p (empty rows are skipped by construction)
__device__ inline int row_of_entry(const int *ptr_lds, int rows, int p) {
  int lo = 0, hi = rows;  // invariant: ptr_lds[lo] <= p < ptr_lds[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr_lds[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// lower bound of column c in the ascending indices idx[a .. b): the caller checks that it is inside and holds c
__device__ inline int find_column(const int *__restrict__ idx, int a, int b, int c) {
  while (a < b) {
    const int mid = (a + b) >> 1;
    if (idx[mid] < c) a = mid + 1; else b = mid;
  }
  return a;
}

// row pointers and column indices of two rows images equal?  one flag
__global__ __launch_bounds__(256) void same_pattern_kernel(int64_t n, int64_t nnz, const int *__restrict__ p1,
                                                           const int *__restrict__ p2, const int *__restrict__ i1,
                                                           const int *__restrict__ i2, int *__restrict__ differ) {
  bool bad = false;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nnz + n + 1; k += (int64_t)gridDim.x * blockDim.x) {
    if (k < nnz) bad |= i1[k] != i2[k];
    else bad |= p1[k - nnz] != p2[k - nnz];
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) *differ = 1;
}

// A == A^T of a complex rows image: every off-diagonal entry (r, c) looks entry (c, r) up by bisection in row c and
// compares the 16 bytes of the two values
__global__ __launch_bounds__(kTileRows) void complex_symmetric_kernel(int64_t n, const int *__restrict__ rowptr,
                                                                      const int *__restrict__ colidx,
                                                                      const double2 *__restrict__ val,
                                                                      int *__restrict__ differ) {
  __shared__ int ptr_lds[kTileRows + 1];
  const int64_t r0 = (int64_t)blockIdx.x * kTileRows;
  const int rows = stage_row_pointers(rowptr, n, r0, ptr_lds);
  bool bad = false;
  for (int p = ptr_lds[0] + (int)threadIdx.x; p < ptr_lds[rows]; p += kTileRows) {
    const int r = (int)r0 + row_of_entry(ptr_lds, rows, p);
    const int c = colidx[p];
    if (c == r) continue;
    if (c >= n) { bad = true; continue; }  // (a rectangular image never gets here; the guard keeps the reads in bounds)
    const int a = rowptr[c], b = rowptr[c + 1];
    const int q = find_column(colidx, a, b, r);
    if (q >= b || colidx[q] != r) { bad = true; continue; }
    const double2 v = val[p], w = val[q];
    bad |= __double_as_longlong(v.x) != __double_as_longlong(w.x) || __double_as_longlong(v.y) != __double_as_longlong(w.y);
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) *differ = 1;
}

// The diagonal of a complex rows image, one thread per row: swap[r] = |im a_rr| > |re a_rr| (the two real equations of
// complex row r change places, umfpack_zi.hip) when swap is given, else diag[r] = a_rr, (0, 0) where no diagonal entry
// is stored.
__global__ __launch_bounds__(256) void complex_diagonal_kernel(int64_t n, const int *__restrict__ rowptr,
                                                               const int *__restrict__ colidx,
                                                               const double2 *__restrict__ val, char *__restrict__ swap,
                                                               double2 *__restrict__ diag) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int a = rowptr[r], b = rowptr[r + 1];
  const int q = find_column(colidx, a, b, (int)r);
  double2 v = make_double2(0.0, 0.0);
  if (q < b && colidx[q] == (int)r) v = val[q];
  if (swap) swap[r] = fabs(v.y) > fabs(v.x) ? 1 : 0;
  else diag[r] = v;
}

// Rows image of the complex matrix -> rows image of its real embedding with interleaved unknowns (umfpack_zi.hip):
// complex entry k of row r (column c, value re + i im) becomes the entries (2c, 2c + 1) at position 2k of the real rows
// 2r and 2r + 1; row 2r starts at 4 rowptr[r], row 2r + 1 one half block row (2 entries per stored entry) further — the
// layout of the host embed(), transposed to rows.  MODE 0: the block [[re, -im], [im, re]]; MODE 1: the same with the two
// rows exchanged where swap[r] is set; MODE 2: the symmetric congruence C M(w), w = (u_lo u_hi) a with the two units taken
// in index order, so that entries (r, c) and (c, r) of a symmetric matrix go through the same operations on the same
// operands and get the same bits (every multiply and add separately rounded, as on the host).
// Per complex entry 20 bytes are read (4 + 16, coalesced) and 48 written: two 8-byte index pairs and two 16-byte value
// pairs, consecutive lanes writing consecutive pairs of the same real row.
template <int MODE>
__global__ __launch_bounds__(kTileRows) void embed_rows_kernel(int64_t n, const int *__restrict__ rowptr,
                                                               const int *__restrict__ colidx,
                                                               const double2 *__restrict__ val,
                                                               const char *__restrict__ swap,
                                                               const double2 *__restrict__ unit,
                                                               int64_t *__restrict__ out_ptr, int2 *__restrict__ out_idx,
                                                               double2 *__restrict__ out_val) {
#pragma clang fp contract(off)
  __shared__ int ptr_lds[kTileRows + 1];
  const int64_t r0 = (int64_t)blockIdx.x * kTileRows;
  const int rows = stage_row_pointers(rowptr, n, r0, ptr_lds);
  if ((int)threadIdx.x < rows) {
    const int64_t a = ptr_lds[threadIdx.x], len = ptr_lds[threadIdx.x + 1] - a;
    out_ptr[2 * (r0 + threadIdx.x)] = 4 * a;
    out_ptr[2 * (r0 + threadIdx.x) + 1] = 4 * a + 2 * len;
    if (r0 + threadIdx.x == n - 1) out_ptr[2 * n] = 4 * (a + len);
  }
  for (int p = ptr_lds[0] + (int)threadIdx.x; p < ptr_lds[rows]; p += kTileRows) {
    const int t = row_of_entry(ptr_lds, rows, p);
    const int r = (int)r0 + t;
    const int64_t a = ptr_lds[t], len = ptr_lds[t + 1] - a;
    const int c = colidx[p];
    const double2 v = val[p];
    double2 top, bottom;  // rows 2r and 2r + 1 of the block
    if (MODE == 2) {
      const int lo = r < c ? r : c, hi = r < c ? c : r;
      const double2 ua = unit[lo], ub = unit[hi];
      const double pr = ua.x * ub.x - ua.y * ub.y, pi = ua.x * ub.y + ua.y * ub.x;
      const double wr = pr * v.x - pi * v.y, wi = pr * v.y + pi * v.x;
      top = make_double2(wr, -wi);
      bottom = make_double2(-wi, -wr);
    } else {
      top = make_double2(v.x, -v.y);
      bottom = make_double2(v.y, v.x);
      if (MODE == 1 && swap[r]) {
        const double2 h = top;
        top = bottom;
        bottom = h;
      }
    }
    const int64_t k0 = (4 * a + 2 * ((int64_t)p - a)) >> 1, k1 = k0 + len;  // in units of pairs
    const int2 cols = make_int2(2 * c, 2 * c + 1);
    out_idx[k0] = cols;
    out_idx[k1] = cols;
    out_val[k0] = top;
    out_val[k1] = bottom;
  }
}

unsigned tiles_of(int64_t n) { return (unsigned)((n + kTileRows - 1) / kTileRows); }

bool flag_clear(const DBuf<int> &flag, hipStream_t s) {
  int h = 1;
  SPL_HIP(hipMemcpyAsync(&h, flag.get(), sizeof(int), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  SPL_HIP(hipGetLastError());
  return h == 0;
}

}  // namespace

int handle_status(const Matrix *H, int vw) {
  if (H->row0 != 0 || H->nrows_local != H->nrows_global || H->vw != vw || !H->rowptr.get() ||
      H->nrows_global > 0x7fffffffLL || H->ncols > 0x7fffffffLL)
    return UMFPACK_ERROR_invalid_matrix;
  return UMFPACK_OK;
}

void handle_to_host_csc(const Matrix *H, std::vector<int> &Ap, std::vector<int> &Ai, std::vector<double> *Ax) {
  const size_t nr = (size_t)H->nrows_local, nc = (size_t)H->ncols, nnz = (size_t)H->nnz, vw = (size_t)H->vw;
  std::vector<int> rp(nr + 1), ci(nnz);
  std::vector<double> v(Ax ? nnz * vw : 0);
  SPL_HIP(hipMemcpy(rp.data(), H->rowptr.get(), (nr + 1) * sizeof(int), hipMemcpyDeviceToHost));
  if (nnz) SPL_HIP(hipMemcpy(ci.data(), H->colidx.get(), nnz * sizeof(int), hipMemcpyDeviceToHost));
  if (Ax && nnz) SPL_HIP(hipMemcpy(v.data(), H->val.get(), nnz * vw * sizeof(double), hipMemcpyDeviceToHost));
  // rows image -> columns image by counting; the rows are walked in ascending order, so they ascend inside a column
  Ap.assign(nc + 1, 0);
  Ai.resize(nnz ? nnz : 1);
  if (Ax) Ax->resize(nnz ? nnz * vw : 1);
  for (size_t p = 0; p < nnz; ++p) ++Ap[(size_t)ci[p] + 1];
  for (size_t j = 0; j < nc; ++j) Ap[j + 1] += Ap[j];
  std::vector<int> next(Ap.begin(), Ap.end() - 1);
  for (size_t r = 0; r < nr; ++r)
    for (int p = rp[r]; p < rp[r + 1]; ++p) {
      const size_t q = (size_t)next[(size_t)ci[(size_t)p]]++;
      Ai[q] = (int)r;
      if (Ax) std::memcpy(Ax->data() + q * vw, v.data() + (size_t)p * vw, vw * sizeof(double));
    }
}

void pattern_from_handle(const Matrix *H, DevicePattern &P, hipStream_t s) {
  const size_t nr = (size_t)H->nrows_local, nnz = (size_t)H->nnz;
  P.rowptr.alloc(nr + 1);
  P.colidx.alloc(nnz);
  SPL_HIP(hipMemcpyAsync(P.rowptr.get(), H->rowptr.get(), (nr + 1) * sizeof(int), hipMemcpyDeviceToDevice, s));
  if (nnz) SPL_HIP(hipMemcpyAsync(P.colidx.get(), H->colidx.get(), nnz * sizeof(int), hipMemcpyDeviceToDevice, s));
  SPL_HIP(hipStreamSynchronize(s));
  P.nrows = H->nrows_local;
  P.nnz = H->nnz;
  P.ready.store(true, std::memory_order_release);
}

bool handle_has_pattern(const Matrix *H, DevicePattern &P, const std::vector<int> &Ap, uint64_t ai_hash, hipStream_t s) {
  if (!P.ready.load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> lock(P.mu);
    if (!P.ready.load(std::memory_order_acquire)) {
      // a host-born analysis: its record is of the columns image — one download of H's pattern, once per Symbolic
      std::vector<int> hp, hi;
      handle_to_host_csc(H, hp, hi, nullptr);
      if (hp != Ap || hash_indices(hi.data(), H->nnz) != ai_hash) return false;
      pattern_from_handle(H, P, s);
      return true;
    }
  }
  if (H->nrows_local != P.nrows || H->nnz != P.nnz) return false;
  DBuf<int> differ(1);
  SPL_HIP(hipMemsetAsync(differ.get(), 0, sizeof(int), s));
  const int64_t total = P.nnz + P.nrows + 1;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(same_pattern_kernel, dim3((unsigned)blocks), dim3(256), 0, s, P.nrows, P.nnz, H->rowptr.get(),
                     P.rowptr.get(), H->colidx.get(), P.colidx.get(), differ.get());
  return flag_clear(differ, s);
}

Matrix *clone_handle(const Matrix *H, hipStream_t s) {
  std::unique_ptr<Matrix> C(new Matrix());
  C->device = H->device;
  C->nrows_global = H->nrows_global;
  C->ncols = H->ncols;
  C->row0 = H->row0;
  C->nrows_local = H->nrows_local;
  C->nnz = H->nnz;
  C->vw = H->vw;
  C->max_row_len = H->max_row_len;
  const size_t nr = (size_t)H->nrows_local, nv = (size_t)H->nnz * (size_t)H->vw;
  C->rowptr64.alloc(nr + 1);
  C->rowptr.alloc(nr + 1);
  C->colidx.alloc((size_t)H->nnz);
  C->val.alloc(nv);
  SPL_HIP(hipMemcpyAsync(C->rowptr64.get(), H->rowptr64.get(), (nr + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  SPL_HIP(hipMemcpyAsync(C->rowptr.get(), H->rowptr.get(), (nr + 1) * sizeof(int), hipMemcpyDeviceToDevice, s));
  if (H->nnz) {
    SPL_HIP(hipMemcpyAsync(C->colidx.get(), H->colidx.get(), (size_t)H->nnz * sizeof(int), hipMemcpyDeviceToDevice, s));
    SPL_HIP(hipMemcpyAsync(C->val.get(), H->val.get(), nv * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  return C.release();
}

bool complex_handle_symmetric(const Matrix *H, hipStream_t s) {
  const int64_t n = H->nrows_local;
  if (H->ncols != n) return false;
  DBuf<int> differ(1);
  SPL_HIP(hipMemsetAsync(differ.get(), 0, sizeof(int), s));
  if (n > 0 && H->nnz > 0)
    hipLaunchKernelGGL(complex_symmetric_kernel, dim3(tiles_of(n)), dim3(kTileRows), 0, s, n, H->rowptr.get(),
                       H->colidx.get(), reinterpret_cast<const double2 *>(H->val.get()), differ.get());
  return flag_clear(differ, s);
}

void complex_handle_diagonal(const Matrix *H, bool units, ComplexDiagonal &D, hipStream_t s) {
  const int64_t n = H->nrows_local;
  if (units) D.d_unit.alloc((size_t)2 * n); else D.d_swap.alloc((size_t)n);
  if (n > 0)
    hipLaunchKernelGGL(complex_diagonal_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, H->rowptr.get(),
                       H->colidx.get(), reinterpret_cast<const double2 *>(H->val.get()), D.d_swap.get(),
                       reinterpret_cast<double2 *>(D.d_unit.get()));
  if (units) {
    // The units are computed HERE, from the n diagonal entries, by the function the host route uses: hypot, divide and
    // sqrt of the device library need not round as the host's do, and one different bit in a unit is a different
    // factorisation.  16 n bytes down, 16 n up — the solves need the units on the host anyway.
    D.unit.resize((size_t)2 * n);
    SPL_HIP(hipMemcpyAsync(D.unit.data(), D.d_unit.get(), (size_t)2 * n * sizeof(double), hipMemcpyDeviceToHost, s));
    SPL_HIP(hipStreamSynchronize(s));
    for (int64_t r = 0; r < n; ++r) congruence_unit(D.unit[(size_t)2 * r], D.unit[(size_t)2 * r + 1], &D.unit[(size_t)2 * r]);
    SPL_HIP(hipMemcpyAsync(D.d_unit.get(), D.unit.data(), (size_t)2 * n * sizeof(double), hipMemcpyHostToDevice, s));
  } else {
    D.swap.resize((size_t)n);
    SPL_HIP(hipMemcpyAsync(D.swap.data(), D.d_swap.get(), (size_t)n, hipMemcpyDeviceToHost, s));
  }
  SPL_HIP(hipStreamSynchronize(s));
  SPL_HIP(hipGetLastError());
  D.any_swap = false;
  for (char f : D.swap) D.any_swap |= f != 0;
}

Matrix *embed_handle(const Matrix *H, const char *d_swap, const double *d_unit, hipStream_t s) {
  const int64_t n = H->nrows_local, nnz = H->nnz;
  std::unique_ptr<Matrix> E(new Matrix());
  E->device = H->device;
  E->nrows_global = E->nrows_local = E->ncols = 2 * n;
  E->nnz = 4 * nnz;
  E->rowptr64.alloc((size_t)2 * n + 1);
  E->colidx.alloc((size_t)4 * nnz);
  E->val.alloc((size_t)4 * nnz);
  if (n == 0) {
    SPL_HIP(hipMemsetAsync(E->rowptr64.get(), 0, sizeof(int64_t), s));
  } else {
    const double2 *val = reinterpret_cast<const double2 *>(H->val.get()), *unit = reinterpret_cast<const double2 *>(d_unit);
    int2 *oi = reinterpret_cast<int2 *>(E->colidx.get());
    double2 *ov = reinterpret_cast<double2 *>(E->val.get());
    const dim3 grid(tiles_of(n)), block(kTileRows);
    if (d_unit)
      hipLaunchKernelGGL(embed_rows_kernel<2>, grid, block, 0, s, n, H->rowptr.get(), H->colidx.get(), val, d_swap, unit,
                         E->rowptr64.get(), oi, ov);
    else if (d_swap)
      hipLaunchKernelGGL(embed_rows_kernel<1>, grid, block, 0, s, n, H->rowptr.get(), H->colidx.get(), val, d_swap, unit,
                         E->rowptr64.get(), oi, ov);
    else
      hipLaunchKernelGGL(embed_rows_kernel<0>, grid, block, 0, s, n, H->rowptr.get(), H->colidx.get(), val, d_swap, unit,
                         E->rowptr64.get(), oi, ov);
  }
  finalize_matrix(E.get(), s);  // 32-bit row pointers, longest row; synchronises s
  SPL_HIP(hipGetLastError());
  return E.release();
}

}  // namespace spl

// submatrix.hip — taking a device-resident handle apart: the window A[r0 : r0 + nr, c0 : c0 + nc] (what the signature
// and the two guards of `subMatrix`, Sparse.hs:704-729, mean) and the selection C[i, j] = A[I[i], J[j]].  The inverse of
// the block assembly of assemble_handles.hip, and shaped like it.
//
// A handle holds the ROW-major image.  Both operations are store streams, 12 (real) or 20 (complex) bytes written per
// kept entry, so the work is shaped to the OUTPUT: a group of G = 1, 2, 4 ... 64 lanes takes one result row, consecutive
// groups take consecutive rows, the host picks G from the mean row length.  Pointer arithmetic is 64-bit throughout; row
// lengths and dimensions fit 32 bits.  Values are moved as bits.  Nothing is handed out by atomics: where an entry
// lands depends on the operands only.
//
// Bytes moved per kept entry of a window: 12 / 20 read, 12 / 20 written; per result row 16 read (two pointers) and
// about 2 log2(len / G) index probes of the bisection, 12 written (length, first position) and read again, 8 written
// (pointer).  A window of whole rows (c0 == 0, nc == ncols) searches nothing, scans nothing and is two device-to-device
// copies behind a pointer shift.  A selection reads the indices of its source rows twice (count, copy) and looks every
// one up in a column map of 4 ncols bytes, which stays in the caches.
#include "row_groups.hpp"

namespace spl {

namespace {

// ---- window -------------------------------------------------------------------------------------------------------
// Result row r is the entries of source row r0 + r whose column lies in [c0, c1): the run between lower_bound(c0) and
// lower_bound(c1) of the row's ascending indices, found by the group's bisection (run_in_row of row_groups.hpp).
// first[r] keeps where the run starts: the copy pass (run_copy_kernel there) does not search again.
template <int G>
__global__ __launch_bounds__(kRowThreads) void window_len_kernel(const int64_t *__restrict__ Ap,
                                                                 const int *__restrict__ Aj, int64_t r0, int64_t nr,
                                                                 int c0, int c1, int *__restrict__ len,
                                                                 int64_t *__restrict__ first) {
  constexpr int kGroups = kRowThreads / G;
  const int lane = threadIdx.x % G;
  int64_t r = (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  for (; r < nr; r += stride) {
    const int64_t s = Ap[r0 + r];
    int n;
    int64_t p;
    run_in_row<G>(Aj, s, (int)(Ap[r0 + r + 1] - s), lane, c0, c1, &n, &p);  // every lane of the group is here
    if (lane == 0) {
      len[r] = n;
      first[r] = p;
    }
  }
}

// whole rows: Cp[i] = Ap[r0 + i] - Ap[r0], i <= nr
__global__ __launch_bounds__(kRowThreads) void shift_pointers_kernel(const int64_t *__restrict__ Ap, int64_t r0,
                                                                     int64_t nr, int64_t *__restrict__ Cp) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  const int64_t base = Ap[r0];
  for (; i <= nr; i += stride) Cp[i] = Ap[r0 + i] - base;
}

// ---- select -------------------------------------------------------------------------------------------------------
// What the checks of the two index arrays leave behind (one 32-byte read-back)
struct SelectFlags {
  unsigned long long bad_row, bad_col;  // smallest offending position, ~0 when none
  int repeated, descends;               // J: a column named twice; J[k - 1] >= J[k] somewhere
  int pad[2];
};

// I: every entry in [0, nrows), compared in the source width, and narrowed to rows[]
template <typename T>
__global__ __launch_bounds__(kRowThreads) void check_rows_kernel(const T *__restrict__ I, int64_t nI, int64_t nrows,
                                                                 int *__restrict__ rows, SelectFlags *__restrict__ f) {
  int64_t k = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; k < nI; k += stride) {
    const T i = I[k];
    const bool ok = i >= 0 && i < (T)nrows;
    rows[k] = ok ? (int)i : 0;
    if (!ok) atomicMin(&f->bad_row, (unsigned long long)k);
  }
}

// J: map[J[k]] = k over a map filled with -1.  A slot that was taken already names a repeated column, an entry outside
// [0, ncols) records its position; whether J ascends is seen on the way (then the result rows need no sort)
template <typename T>
__global__ __launch_bounds__(kRowThreads) void scatter_cols_kernel(const T *__restrict__ J, int64_t nJ, int64_t ncols,
                                                                   int *__restrict__ map, SelectFlags *__restrict__ f) {
  int64_t k = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; k < nJ; k += stride) {
    const T j = J[k];
    if (j < 0 || j >= (T)ncols) {
      atomicMin(&f->bad_col, (unsigned long long)k);
      continue;
    }
    if (atomicCAS(&map[j], -1, (int)k) != -1) f->repeated = 1;  // every writer stores the same 1
    if (k > 0 && J[k - 1] >= j) f->descends = 1;
  }
}

// source row of result row r; kept(c): the new column of old column c, or -1
__device__ inline int64_t source_row(const int *__restrict__ rows, int64_t r) { return rows ? (int64_t)rows[r] : r; }

template <int G>
__global__ __launch_bounds__(kRowThreads) void select_len_kernel(const int64_t *__restrict__ Ap,
                                                                 const int *__restrict__ Aj,
                                                                 const int *__restrict__ rows,
                                                                 const int *__restrict__ map, int64_t nI,
                                                                 int *__restrict__ len) {
  constexpr int kGroups = kRowThreads / G;
  const int lane = threadIdx.x % G;
  int64_t r = (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  for (; r < nI; r += stride) {
    const int64_t src = source_row(rows, r);
    const int64_t s = Ap[src], e = Ap[src + 1];
    int n = 0;
    if (map) {
      for (int64_t p = s + lane; p < e; p += G) n += map[Aj[p]] >= 0;
      n = group_sum<G>(n);
    } else {
      n = (int)(e - s);
    }
    if (lane == 0) len[r] = n;
  }
}

// The copy keeps the source order inside the row.  The group walks the source row G entries at a time; in every step
// the lanes that keep their entry are counted by a ballot, a lane's place is the count of kept lanes below it, and the
// row's write position moves on by the step's total.  The steps of a row are the same for all lanes of its group (the
// loop bound does not depend on the lane), so the group's bits of the ballot are complete whatever the other groups of
// the wavefront are doing.
template <int G, int VW>
__global__ __launch_bounds__(kRowThreads) void select_copy_kernel(const int64_t *__restrict__ Ap,
                                                                  const int *__restrict__ Aj,
                                                                  const double *__restrict__ Ax,
                                                                  const int *__restrict__ rows,
                                                                  const int *__restrict__ map, int64_t nI,
                                                                  const int64_t *__restrict__ Cp, int *__restrict__ Cj,
                                                                  double *__restrict__ Cx) {
  constexpr int kGroups = kRowThreads / G;
  constexpr unsigned long long kGroupMask = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
  const int lane = threadIdx.x % G;
  const int shift = (threadIdx.x & 63) - lane;  // the group's first lane in its wavefront
  int64_t r = (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  for (; r < nI; r += stride) {
    const int64_t src = source_row(rows, r);
    const int64_t s = Ap[src], e = Ap[src + 1];
    int64_t o = Cp[r];
    for (int64_t base = s; base < e; base += G) {
      const int64_t p = base + lane;
      int c = -1;
      if (p < e) {
        c = Aj[p];
        if (map) c = map[c];
      }
      const unsigned long long bits = (__ballot(c >= 0) >> shift) & kGroupMask;
      if (c >= 0) {
        const int64_t q = o + __popcll(bits & ((1ull << lane) - 1ull));
        Cj[q] = c;
        move_value<VW>(Ax, p, Cx, q);
      }
      o += __popcll(bits);
    }
  }
}

}  // namespace

// C = A[r0 : r0 + nr, c0 : c0 + nc] on the row image of a whole handle; the caller checked the window against A's
// dimensions and set C's dimensions and value kind.  Fills rowptr64 / colidx / val / nnz; synchronises s.
void submatrix_handle(const Matrix *A, int64_t r0, int64_t c0, Matrix *C, hipStream_t s) {
  const int64_t nr = C->nrows_local, nc = C->ncols;
  if (nr == 0 || nc == 0 || A->nnz == 0) {
    empty_result(C, s);
    return;
  }
  C->rowptr64.alloc((size_t)nr + 1);
  if (c0 == 0 && nc == A->ncols) {
    // whole rows: their entries lie one behind the other in A and keep their column indices
    hipLaunchKernelGGL(shift_pointers_kernel, dim3(grid_flat(nr + 1)), dim3(kRowThreads), 0, s, A->rowptr64.get(), r0, nr,
                       C->rowptr64.get());
    SPL_HIP(hipGetLastError());
    int64_t start = 0;
    SPL_HIP(hipMemcpyAsync(&start, A->rowptr64.get() + r0, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    allocate_entries(C, s);  // synchronises: `start` has arrived
    if (C->nnz > 0) {
      SPL_HIP(hipMemcpyAsync(C->colidx.get(), A->colidx.get() + start, (size_t)C->nnz * sizeof(int),
                             hipMemcpyDeviceToDevice, s));
      SPL_HIP(hipMemcpyAsync(C->val.get(), A->val.get() + start * A->vw, (size_t)C->nnz * (size_t)A->vw * sizeof(double),
                             hipMemcpyDeviceToDevice, s));
    }
    SPL_HIP(hipStreamSynchronize(s));
    return;
  }
  DBuf<int> len((size_t)nr);
  DBuf<int64_t> first((size_t)nr);
  const int c1 = (int)(c0 + nc);  // <= ncols < 2^31
  // lanes per row: the length pass cuts the SOURCE rows into pieces, the copy pass walks the kept entries
  const int g1 = group_for((double)A->nnz / (double)A->nrows_local);
  for_group_and_width(g1, C->vw, [&](auto g, auto) {
    hipLaunchKernelGGL((window_len_kernel<decltype(g)::value>), dim3(grid_rows(nr, g)), dim3(kRowThreads), 0, s,
                       A->rowptr64.get(), A->colidx.get(), r0, nr, (int)c0, c1, len.get(), first.get());
  });
  SPL_HIP(hipGetLastError());
  exclusive_scan_i32_to_i64(len.get(), C->rowptr64.get(), nr, s);
  allocate_entries(C, s);
  if (C->nnz > 0) {
    const int g2 = group_for((double)C->nnz / (double)nr);
    for_group_and_width(g2, C->vw, [&](auto g, auto vw) {
      hipLaunchKernelGGL((run_copy_kernel<decltype(g)::value, decltype(vw)::value>), dim3(grid_rows(nr, g)),
                         dim3(kRowThreads), 0, s, A->colidx.get(), A->val.get(), first.get(), nr, (int)c0,
                         C->rowptr64.get(), C->colidx.get(), C->val.get());
    });
    SPL_HIP(hipGetLastError());
  }
  SPL_HIP(hipStreamSynchronize(s));  // `len` and `first` are released on return
}

// C[i, j] = A[I[i], J[j]] on the row image of a whole handle.  d_I / d_J: device arrays of index_width bytes per entry,
// nullptr = all rows / all columns in order (the caller checked the counts then).  C's dimensions (nI x nJ) and value
// kind are set.  SPL_OK: rowptr64 / colidx / val / nnz are filled, source order kept inside every row, and *ascending
// says whether that order ascends (false: the caller sorts the rows).  SPL_ERROR_index_out_of_bounds with *bad = the
// first offending position (I before J); SPL_ERROR_invalid_matrix for a column named twice.  Synchronises s.
int select_handle(const Matrix *A, int index_width, const void *d_I, const void *d_J, Matrix *C, bool *ascending,
                  int64_t *bad, hipStream_t s) {
  const int64_t nI = C->nrows_local, nJ = C->ncols;
  *ascending = true;
  DBuf<int> rows, map;
  if ((d_I && nI > 0) || (d_J && nJ > 0)) {
    DBuf<SelectFlags> flags(1);
    SelectFlags h;
    h.bad_row = h.bad_col = ~0ull;
    h.repeated = h.descends = 0;
    h.pad[0] = h.pad[1] = 0;
    SPL_HIP(hipMemcpyAsync(flags.get(), &h, sizeof(h), hipMemcpyHostToDevice, s));
    if (d_I && nI > 0) {
      rows.alloc((size_t)nI);
      if (index_width == 8)
        hipLaunchKernelGGL((check_rows_kernel<int64_t>), dim3(grid_flat(nI)), dim3(kRowThreads), 0, s,
                           static_cast<const int64_t *>(d_I), nI, A->nrows_local, rows.get(), flags.get());
      else
        hipLaunchKernelGGL((check_rows_kernel<int>), dim3(grid_flat(nI)), dim3(kRowThreads), 0, s,
                           static_cast<const int *>(d_I), nI, A->nrows_local, rows.get(), flags.get());
    }
    if (d_J && nJ > 0) {
      map.alloc((size_t)A->ncols);
      SPL_HIP(hipMemsetAsync(map.get(), 0xFF, (size_t)A->ncols * sizeof(int), s));  // -1 everywhere
      if (index_width == 8)
        hipLaunchKernelGGL((scatter_cols_kernel<int64_t>), dim3(grid_flat(nJ)), dim3(kRowThreads), 0, s,
                           static_cast<const int64_t *>(d_J), nJ, A->ncols, map.get(), flags.get());
      else
        hipLaunchKernelGGL((scatter_cols_kernel<int>), dim3(grid_flat(nJ)), dim3(kRowThreads), 0, s,
                           static_cast<const int *>(d_J), nJ, A->ncols, map.get(), flags.get());
    }
    SPL_HIP(hipGetLastError());
    SPL_HIP(hipMemcpyAsync(&h, flags.get(), sizeof(h), hipMemcpyDeviceToHost, s));
    SPL_HIP(hipStreamSynchronize(s));
    if (h.bad_row != ~0ull || h.bad_col != ~0ull) {
      if (bad) *bad = (int64_t)(h.bad_row != ~0ull ? h.bad_row : h.bad_col);
      return SPL_ERROR_index_out_of_bounds;
    }
    if (h.repeated) return SPL_ERROR_invalid_matrix;
    *ascending = !h.descends;
  }
  if (nI == 0 || nJ == 0 || A->nnz == 0) {
    empty_result(C, s);
    SPL_HIP(hipStreamSynchronize(s));
    return SPL_OK;
  }
  const int *d_rows = rows.get(), *d_map = map.get();  // nullptr where the array was not given
  DBuf<int> len((size_t)nI);
  C->rowptr64.alloc((size_t)nI + 1);
  // lanes per row, both passes walk the source rows: their mean length (that of A; I may name any of them)
  const int g = group_for((double)A->nnz / (double)A->nrows_local);
  for_group_and_width(g, C->vw, [&](auto gc, auto) {
    hipLaunchKernelGGL((select_len_kernel<decltype(gc)::value>), dim3(grid_rows(nI, gc)), dim3(kRowThreads), 0, s,
                       A->rowptr64.get(), A->colidx.get(), d_rows, d_map, nI, len.get());
  });
  SPL_HIP(hipGetLastError());
  exclusive_scan_i32_to_i64(len.get(), C->rowptr64.get(), nI, s);
  allocate_entries(C, s);
  if (C->nnz > 0) {
    for_group_and_width(g, C->vw, [&](auto gc, auto vw) {
      hipLaunchKernelGGL((select_copy_kernel<decltype(gc)::value, decltype(vw)::value>), dim3(grid_rows(nI, gc)),
                         dim3(kRowThreads), 0, s, A->rowptr64.get(), A->colidx.get(), A->val.get(), d_rows, d_map, nI,
                         C->rowptr64.get(), C->colidx.get(), C->val.get());
    });
    SPL_HIP(hipGetLastError());
  }
  SPL_HIP(hipStreamSynchronize(s));  // `rows`, `map` and `len` are released on return
  return SPL_OK;
}

}  // namespace spl

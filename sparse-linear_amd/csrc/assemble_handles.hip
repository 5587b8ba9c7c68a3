// assemble_handles.hip — the structural constructors on device-resident handles: kronecker (Sparse.hs:597-634),
// hcat / vcat / fromBlocks / fromBlocksDiag / blockDiag (Sparse.hs:500-595, 661-667), takeDiag (Sparse.hs:640-650),
// diag / ident (Sparse.hs:652-659, 669-671).
//
// A handle holds the ROW-major image: its (rowptr64, colidx, val) are the CSC fields of the transpose.  Every kernel
// here walks that image; what the reference does per column these do per row, on the transposes (see the comment
// above each entry point in abi.hip for why that gives the reference's result).  The host-tuple calls spl_kronecker,
// spl_assemble_blocks and spl_take_diag run the same kernels: a caller's CSC 5-tuple, uploaded as it is, is the row image
// of its transpose, and all three operations commute with transposition (blocks with their offsets exchanged).
//
// All of them are store streams: 12 (real) or 20 (complex) bytes written per entry, the operands small and read
// through the caches.  The work is therefore shaped to the OUTPUT: a group of G = 1, 2, 4 ... 64 lanes takes one result
// row, consecutive groups take consecutive rows, and since the rows of the result lie one behind the other the lanes
// of a wavefront write one contiguous range whatever G is.  The host picks G from the mean row length, so a row of
// three entries costs four lanes, not a wavefront.  Pointer arithmetic is 64-bit throughout; row lengths and
// dimensions fit 32 bits (the callers refuse dimensions of 2^31 and more).
#include <algorithm>

#include "row_groups.hpp"

namespace spl {

namespace {

// ---- kronecker ------------------------------------------------------------------------------------------------
// Row r = ra * nrowsB + rb of C = A (x) B is, for every entry (ca, a) of row ra of A in order and every entry (cb, b)
// of row rb of B in order, the entry (ca * ncolsB + cb, b * a); it starts at Ap[ra] * nnzB + lenA(ra) * Bp[rb] (the
// rows of the blocks above hold Ap[ra] * nnzB entries, the rows above inside the block lenA(ra) * Bp[rb]).  So there is
// nothing to count and nothing to scan: one kernel writes pointers, indices and values.
// A group of G lanes takes a row; lane l writes entries l, l + G, ...  Entry e is the pair (e / lenB, e % lenB): ONE
// 32-bit division per lane and row gives the lane's first pair, and the step (G / lenB, G % lenB) comes from the
// group's last lane, whose first pair is ((G-1) / lenB, (G-1) % lenB), by a shuffle.  After that the pair advances by
// counters.  The rows themselves advance by counters as well (the grid's stride as a pair, from the host).
template <int G, int VW>
__global__ __launch_bounds__(kRowThreads) void kron_rows_kernel(
    const int64_t *__restrict__ Ap, const int *__restrict__ Aj, const double *__restrict__ Ax,
    const int64_t *__restrict__ Bp, const int *__restrict__ Bj, const double *__restrict__ Bx, unsigned nrowsB,
    unsigned ncolsB, int64_t nnzB, int64_t nrowsC, int64_t nnzC, unsigned stride_a, unsigned stride_b,
    int64_t *__restrict__ Cp, int *__restrict__ Cj, double *__restrict__ Cx) {
  constexpr int kGroups = kRowThreads / G;
  const unsigned lane = threadIdx.x % G;
  int64_t r = (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;  // == stride_a * nrowsB + stride_b
  unsigned ra = (unsigned)r / nrowsB, rb = (unsigned)r - ra * nrowsB;  // r < 2^24 here; once per lane, not per row
  for (; r < nrowsC; r += stride) {
    const int64_t pa = Ap[ra], pb = Bp[rb];
    const unsigned lenA = (unsigned)(Ap[ra + 1] - pa), lenB = (unsigned)(Bp[rb + 1] - pb);
    const int64_t base = pa * nnzB + (int64_t)lenA * pb;
    const unsigned len = lenA * lenB;  // <= ncolsA * ncolsB < 2^31
    if (lane == 0) {
      Cp[r] = base;
      if (r == nrowsC - 1) Cp[nrowsC] = nnzC;
    }
    // the division and the shuffle before any branch on the row's length: every lane of the group takes part
    const unsigned div = lenB ? lenB : 1u;
    unsigned ea = lane / div, eb = lane - ea * div;
    unsigned sa, sb;
    if (G == 1) {
      sa = ea; sb = eb;
    } else {
      sa = (unsigned)__shfl((int)ea, G - 1, G);
      sb = (unsigned)__shfl((int)eb, G - 1, G);
    }
    if (++sb == div) { sb = 0; ++sa; }  // (G - 1) + 1
    for (unsigned e = lane; e < len; e += G) {
      const int64_t ka = pa + ea, kb = pb + eb, o = base + e;
      Cj[o] = (int)((unsigned)Aj[ka] * ncolsB + (unsigned)Bj[kb]);
      if (VW == 1) {
        store_value<1>(Cx, o, Bx[kb] * Ax[ka], 0.0);  // U.map (* a) bs
      } else {
        // (br :+ bi) * (ar :+ ai) = (br*ar - bi*ai) :+ (br*ai + bi*ar), every operation rounded once
        const double ar = Ax[2 * ka], ai = Ax[2 * ka + 1], br = Bx[2 * kb], bi = Bx[2 * kb + 1];
        store_value<2>(Cx, o, br * ar - bi * ai, br * ai + bi * ar);
      }
      ea += sa;
      eb += sb;
      if (eb >= lenB) { eb -= lenB; ++ea; }
    }
    ra += stride_a;
    rb += stride_b;
    if (rb >= nrowsB) { rb -= nrowsB; ++ra; }
  }
}

// ---- block assembly -------------------------------------------------------------------------------------------
// What the device knows of a placed block, and the table that says which blocks cover a result row: the rows are cut
// at every block boundary into intervals [cut[i], cut[i+1]), and list[lptr[i] .. lptr[i+1]) names the blocks covering
// interval i by ascending column offset.  A group of lanes per result row finds its interval by bisection and walks
// that list: the length pass adds the blocks' row lengths, the copy pass puts each block's row behind its
// predecessors'.  Every entry comes from exactly one block and the rectangles do not overlap, so the rows ascend and
// the result does not depend on the order the blocks were listed in; no atomics, no cursors.
struct PlacedBlock {
  const int64_t *p;
  const int *j;
  const double *x;
  int row_off, col_off;
};

__device__ inline int find_interval(const int *__restrict__ cut, int nint, int r) {
  int lo = 0, hi = nint;  // cut[lo] <= r < cut[hi]; cut[0] == 0, cut[nint] == nrowsC
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (cut[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

template <int G>
__global__ __launch_bounds__(kRowThreads) void blocks_len_kernel(const PlacedBlock *__restrict__ blk,
                                                                 const int *__restrict__ cut, int nint,
                                                                 const int *__restrict__ lptr,
                                                                 const int *__restrict__ list, int nrowsC,
                                                                 int *__restrict__ len) {
  constexpr int kGroups = kRowThreads / G;
  const int lane = threadIdx.x % G;
  int64_t r = (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  for (; r < nrowsC; r += stride) {
    const int i = find_interval(cut, nint, (int)r);
    int n = 0;
    for (int t = lptr[i] + lane; t < lptr[i + 1]; t += G) {
      const PlacedBlock b = blk[list[t]];
      const int64_t *p = b.p + ((int)r - b.row_off);
      n += (int)(p[1] - p[0]);
    }
    n = group_sum<G>(n);  // all lanes of the group are here: r is theirs in common
    if (lane == 0) len[r] = n;  // <= ncolsC < 2^31
  }
}

template <int G, int VW>
__global__ __launch_bounds__(kRowThreads) void blocks_copy_rows_kernel(const PlacedBlock *__restrict__ blk,
                                                                       const int *__restrict__ cut, int nint,
                                                                       const int *__restrict__ lptr,
                                                                       const int *__restrict__ list, int nrowsC,
                                                                       const int64_t *__restrict__ Cp,
                                                                       int *__restrict__ Cj, double *__restrict__ Cx) {
  constexpr int kGroups = kRowThreads / G;
  const int lane = threadIdx.x % G;
  int64_t r = (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  for (; r < nrowsC; r += stride) {
    const int i = find_interval(cut, nint, (int)r);
    int64_t o = Cp[r];
    for (int t = lptr[i]; t < lptr[i + 1]; ++t) {
      const PlacedBlock b = blk[list[t]];
      const int64_t *p = b.p + ((int)r - b.row_off);
      const int64_t s = p[0];
      const int n = (int)(p[1] - s);
      for (int e = lane; e < n; e += G) {
        Cj[o + e] = b.j[s + e] + b.col_off;
        if (VW == 1) store_value<1>(Cx, o + e, b.x[s + e], 0.0);
        else store_value<2>(Cx, o + e, b.x[2 * (s + e)], b.x[2 * (s + e) + 1]);
      }
      o += n;
    }
  }
}

// ---- diagonals --------------------------------------------------------------------------------------------------
// d[c] = A[c, c] or 0: 8 lanes search row c of the row image (at most one hit); on 64-bit pointers, real or packed
// complex values
template <int VW>
__global__ __launch_bounds__(kRowThreads) void take_diag_rows_kernel(const int64_t *__restrict__ Ap,
                                                                     const int *__restrict__ Aj,
                                                                     const double *__restrict__ Ax, int64_t n,
                                                                     double *__restrict__ d) {
  const int64_t c = ((int64_t)blockIdx.x * kRowThreads + threadIdx.x) >> 3;
  const int part = threadIdx.x & 7;
  double v[VW];
#pragma unroll
  for (int q = 0; q < VW; ++q) v[q] = 0.0;
  if (c < n)
    for (int64_t p = Ap[c] + part; p < Ap[c + 1]; p += 8)
      if (Aj[p] == (int)c) {
#pragma unroll
        for (int q = 0; q < VW; ++q) v[q] = Ax[VW * p + q];
      }
  // exactly one lane can hold a hit; OR the bit patterns together (0.0 is all-zero bits)
#pragma unroll
  for (int q = 0; q < VW; ++q) {
    unsigned long long bits = (unsigned long long)__double_as_longlong(v[q]);
    bits |= __shfl_xor(bits, 1, 64);
    bits |= __shfl_xor(bits, 2, 64);
    bits |= __shfl_xor(bits, 4, 64);
    if (c < n && part == 0) d[VW * c + q] = __longlong_as_double((long long)bits);
  }
}

// diag (Sparse.hs:652-659): pointers 0 .. n, indices 0 .. n-1, the values copied — or ones (ident) when there are none
template <int VW>
__global__ __launch_bounds__(kRowThreads) void diag_kernel(int64_t n, const double *__restrict__ values,
                                                           int64_t *__restrict__ Cp, int *__restrict__ Cj,
                                                           double *__restrict__ Cx) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; i <= n; i += stride) {
    Cp[i] = i;
    if (i < n) {
      Cj[i] = (int)i;
      if (VW == 1) store_value<1>(Cx, i, values ? values[i] : 1.0, 0.0);
      else store_value<2>(Cx, i, values ? values[2 * i] : 1.0, values ? values[2 * i + 1] : 0.0);
    }
  }
}

}  // namespace

// C = A (x) B on the row images of two whole handles of one value kind; C's dimensions are set and fit 31 bits (the
// caller checked).  Fills C->rowptr64 / colidx / val / nnz; nothing is counted on the device and nothing waits.
void kronecker_handles(const Matrix *A, const Matrix *B, Matrix *C, hipStream_t s) {
  const int64_t nrowsC = C->nrows_local;
  const int64_t nnzC = A->nnz * B->nnz;
  allocate_result(C, nnzC);
  if (nrowsC == 0) {
    zero_pointers(C, s);
    return;
  }
  const int group = group_for((double)nnzC / (double)nrowsC);
  const unsigned grid = grid_rows(nrowsC, group);
  const int64_t stride = (int64_t)grid * (kRowThreads / group);
  const int64_t nrowsB = B->nrows_local;  // > 0, as nrowsC is
  const unsigned stride_a = (unsigned)(stride / nrowsB), stride_b = (unsigned)(stride % nrowsB);
  for_group_and_width(group, C->vw, [&](auto g, auto vw) {
    hipLaunchKernelGGL((kron_rows_kernel<decltype(g)::value, decltype(vw)::value>), dim3(grid), dim3(kRowThreads), 0, s,
                       A->rowptr64.get(), A->colidx.get(), A->val.get(), B->rowptr64.get(), B->colidx.get(),
                       B->val.get(), (unsigned)B->nrows_local, (unsigned)B->ncols, B->nnz, nrowsC, nnzC, stride_a,
                       stride_b, C->rowptr64.get(), C->colidx.get(), C->val.get());
  });
  SPL_HIP(hipGetLastError());
}

// The interval table of k placed rectangles (host).  SPL_ERROR_dimension_mismatch when one leaves the result or two
// overlap; rectangles without rows or columns hold nothing and are left out.
int blocks_table(int nblocks, const Matrix *const *blk, const int64_t *row_off, const int64_t *col_off, int64_t nrowsC,
                 int64_t ncolsC, std::vector<int> &cut, std::vector<int> &lptr, std::vector<int> &list) {
  std::vector<int> live;
  for (int b = 0; b < nblocks; ++b) {
    const int64_t h = blk[b]->nrows_global, w = blk[b]->ncols;
    if (row_off[b] < 0 || col_off[b] < 0 || row_off[b] > nrowsC - h || col_off[b] > ncolsC - w)
      return SPL_ERROR_dimension_mismatch;
    if (h > 0 && w > 0) live.push_back(b);
  }
  cut.clear();
  cut.push_back(0);
  cut.push_back((int)nrowsC);
  for (int b : live) {
    cut.push_back((int)row_off[b]);
    cut.push_back((int)(row_off[b] + blk[b]->nrows_global));
  }
  std::sort(cut.begin(), cut.end());
  cut.erase(std::unique(cut.begin(), cut.end()), cut.end());  // nrowsC == 0: the one cut 0, no interval
  const int nint = (int)cut.size() - 1;
  // blocks by ascending column offset, dealt to the intervals they cover: every list comes out in that order
  std::sort(live.begin(), live.end(), [&](int a, int b) { return col_off[a] < col_off[b]; });
  std::vector<int> first(live.size()), last(live.size());
  lptr.assign((size_t)nint + 1, 0);
  for (size_t t = 0; t < live.size(); ++t) {
    const int b = live[t];
    first[t] = (int)(std::lower_bound(cut.begin(), cut.end(), (int)row_off[b]) - cut.begin());
    last[t] = (int)(std::lower_bound(cut.begin(), cut.end(), (int)(row_off[b] + blk[b]->nrows_global)) - cut.begin());
    for (int i = first[t]; i < last[t]; ++i) ++lptr[(size_t)i + 1];
  }
  for (int i = 0; i < nint; ++i) lptr[(size_t)i + 1] += lptr[(size_t)i];
  list.assign((size_t)(nint > 0 ? lptr[(size_t)nint] : 0), 0);
  std::vector<int> fill(lptr.begin(), lptr.end());
  for (size_t t = 0; t < live.size(); ++t)
    for (int i = first[t]; i < last[t]; ++i) list[(size_t)fill[(size_t)i]++] = live[t];
  // neighbours in a list share rows: their column ranges must not
  for (int i = 0; i < nint; ++i)
    for (int t = lptr[(size_t)i] + 1; t < lptr[(size_t)i + 1]; ++t) {
      const int a = list[(size_t)t - 1], b = list[(size_t)t];
      if (col_off[a] + blk[a]->ncols > col_off[b]) return SPL_ERROR_dimension_mismatch;
    }
  return SPL_OK;
}

// Places the blocks of a table that blocks_table accepted: three launches whatever nblocks is (lengths, the scan,
// the copy), no host synchronisation — nnz(C) is the sum of the blocks'.
void assemble_handles(int nblocks, const Matrix *const *blk, const int64_t *row_off, const int64_t *col_off,
                      const std::vector<int> &cut, const std::vector<int> &lptr, const std::vector<int> &list, Matrix *C,
                      hipStream_t s) {
  const int64_t nrowsC = C->nrows_local;
  const int nint = (int)cut.size() - 1;
  int64_t nnzC = 0;
  for (int b = 0; b < nblocks; ++b) nnzC += blk[b]->nnz;
  allocate_result(C, nnzC);
  if (nrowsC == 0 || nnzC == 0) {
    zero_pointers(C, s);
    return;
  }
  std::vector<PlacedBlock> hb((size_t)nblocks);
  for (int b = 0; b < nblocks; ++b)
    hb[(size_t)b] = PlacedBlock{blk[b]->rowptr64.get(), blk[b]->colidx.get(), blk[b]->val.get(), (int)row_off[b],
                                (int)col_off[b]};
  // one upload: the blocks, then cut | lptr | list as ints
  const size_t nb_bytes = hb.size() * sizeof(PlacedBlock);
  const size_t nints = cut.size() + lptr.size() + list.size();
  DBuf<unsigned char> table(nb_bytes + nints * sizeof(int));
  std::vector<unsigned char> host(nb_bytes + nints * sizeof(int));
  memcpy(host.data(), hb.data(), nb_bytes);
  int *hi = reinterpret_cast<int *>(host.data() + nb_bytes);
  std::copy(cut.begin(), cut.end(), hi);
  std::copy(lptr.begin(), lptr.end(), hi + cut.size());
  std::copy(list.begin(), list.end(), hi + cut.size() + lptr.size());
  SPL_HIP(hipMemcpyAsync(table.get(), host.data(), host.size(), hipMemcpyHostToDevice, s));
  SPL_HIP(hipStreamSynchronize(s));  // `host` is pageable and leaves scope; the copy is a few kilobytes
  const PlacedBlock *d_blk = reinterpret_cast<const PlacedBlock *>(table.get());
  const int *d_cut = reinterpret_cast<const int *>(table.get() + nb_bytes);
  const int *d_lptr = d_cut + cut.size(), *d_list = d_lptr + lptr.size();

  DBuf<int> len((size_t)nrowsC);
  // lanes per row: the length pass walks the list (mean covering blocks per row), the copy pass the entries
  int64_t covered = 0;
  for (int i = 0; i < nint; ++i)
    covered += (int64_t)(lptr[(size_t)i + 1] - lptr[(size_t)i]) * (cut[(size_t)i + 1] - cut[(size_t)i]);
  const int g1 = group_for((double)covered / (double)nrowsC);
  const int g2 = group_for((double)nnzC / (double)nrowsC);
  for_group_and_width(g1, C->vw, [&](auto g, auto) {
    hipLaunchKernelGGL((blocks_len_kernel<decltype(g)::value>), dim3(grid_rows(nrowsC, g)), dim3(kRowThreads), 0, s,
                       d_blk, d_cut, nint, d_lptr, d_list, (int)nrowsC, len.get());
  });
  exclusive_scan_i32_to_i64(len.get(), C->rowptr64.get(), nrowsC, s);
  for_group_and_width(g2, C->vw, [&](auto g, auto vw) {
    hipLaunchKernelGGL((blocks_copy_rows_kernel<decltype(g)::value, decltype(vw)::value>), dim3(grid_rows(nrowsC, g)),
                       dim3(kRowThreads), 0, s, d_blk, d_cut, nint, d_lptr, d_list, (int)nrowsC, C->rowptr64.get(),
                       C->colidx.get(), C->val.get());
  });
  SPL_HIP(hipGetLastError());
  SPL_HIP(hipStreamSynchronize(s));  // `len` and `table` are released on return
}

// d[c] = A[c, c] (or 0), c < n = min(nrows, ncols), enqueued on s; d holds n entries of the handle's value kind
void take_diag_handle(const Matrix *A, int64_t n, double *d, hipStream_t s) {
  if (n <= 0) return;
  const unsigned grid = (unsigned)(((size_t)n * 8 + kRowThreads - 1) / kRowThreads);
  if (A->vw == 1)
    hipLaunchKernelGGL((take_diag_rows_kernel<1>), dim3(grid), dim3(kRowThreads), 0, s, A->rowptr64.get(),
                       A->colidx.get(), A->val.get(), n, d);
  else
    hipLaunchKernelGGL((take_diag_rows_kernel<2>), dim3(grid), dim3(kRowThreads), 0, s, A->rowptr64.get(),
                       A->colidx.get(), A->val.get(), n, d);
  SPL_HIP(hipGetLastError());
}

// the n x n diagonal matrix of n values in device memory (nullptr: ones); C's dimensions and value kind are set
void diag_handle(const double *d_values, Matrix *C, hipStream_t s) {
  const int64_t n = C->nrows_local;
  allocate_result(C, n);
  const unsigned blocks = grid_flat(n + 1);
  if (C->vw == 1)
    hipLaunchKernelGGL((diag_kernel<1>), dim3(blocks), dim3(kRowThreads), 0, s, n, d_values,
                       C->rowptr64.get(), C->colidx.get(), C->val.get());
  else
    hipLaunchKernelGGL((diag_kernel<2>), dim3(blocks), dim3(kRowThreads), 0, s, n, d_values,
                       C->rowptr64.get(), C->colidx.get(), C->val.get());
  SPL_HIP(hipGetLastError());
}

}  // namespace spl

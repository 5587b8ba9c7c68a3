// row_groups.hpp — the launch frame of the kernels that give every result row a group of lanes (assemble_handles.hip,
// submatrix.hip, entrywise.hip).  A group of G = 1, 2, 4 ... 64 lanes takes one result row, consecutive groups take consecutive rows,
// and the host picks G from the mean row length; VW is the doubles per stored value (1 real, 2 packed complex).
#pragma once

#include <type_traits>

#include "common.hpp"

namespace spl {

constexpr int kRowThreads = 256;  // threads per workgroup of every kernel launched through this frame

inline unsigned grid_rows(int64_t rows, int group, int64_t cap = 1 << 16) {
  const int64_t per_block = kRowThreads / group;
  int64_t b = (rows + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (unsigned)b;
}

inline unsigned grid_flat(int64_t n, int64_t cap = 1 << 16) {
  int64_t b = (n + kRowThreads - 1) / kRowThreads;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (unsigned)b;
}

// smallest power of two >= mean (1 ... 64): the lanes one result row gets
inline int group_for(double mean) {
  int g = 1;
  while (g < 64 && (double)g < mean) g <<= 1;
  return g;
}

// The runtime (group, vw) as compile-time constants: f(G, VW) receives two std::integral_constant<int, ...> values and
// launches kernel<decltype(G)::value, decltype(VW)::value>.  A kernel that does not depend on VW ignores the second.
template <typename F>
void for_group_and_width(int group, int vw, F &&f) {
  auto with_group = [&](auto g) {
    if (vw == 1) f(g, std::integral_constant<int, 1>{});
    else f(g, std::integral_constant<int, 2>{});
  };
  switch (group) {
    case 1: with_group(std::integral_constant<int, 1>{}); break;
    case 2: with_group(std::integral_constant<int, 2>{}); break;
    case 4: with_group(std::integral_constant<int, 4>{}); break;
    case 8: with_group(std::integral_constant<int, 8>{}); break;
    case 16: with_group(std::integral_constant<int, 16>{}); break;
    case 32: with_group(std::integral_constant<int, 32>{}); break;
    default: with_group(std::integral_constant<int, 64>{}); break;
  }
}

// sum over the G lanes of a group; every lane of the group must be here
template <int G>
__device__ inline int group_sum(int v) {
#pragma unroll
  for (int w = 1; w < G; w <<= 1) v += __shfl_xor(v, w, G);
  return v;
}

// entries of the ascending run j[a .. b) that are < x
__device__ inline int count_less(const int *__restrict__ j, int64_t a, int64_t b, int x) {
  int64_t lo = a, hi = b;  // j[a .. lo) < x <= j[hi .. b)
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (j[mid] < x) lo = mid + 1; else hi = mid;
  }
  return (int)(lo - a);
}

// The run of the ascending row j[s .. s + n) whose indices lie in [c0, c1), between lower_bound(c0) and lower_bound(c1):
// *len entries from position *first on.  The G lanes of the group cut the row into G pieces and bisect one each — "how
// many entries are below x" adds up over the pieces — so a row of 300 entries costs each lane three probes.  Every lane
// of the group must be here, and every lane receives the result.
template <int G>
__device__ inline void run_in_row(const int *__restrict__ j, int64_t s, int n, int lane, int c0, int c1, int *len,
                                  int64_t *first) {
  const int piece = (n + G - 1) / G;
  const int a = min(lane * piece, n), b = min(a + piece, n);  // lane * piece <= 63 * ceil(n / 64) < 2^31
  int below0 = count_less(j, s + a, s + b, c0);
  int below1 = count_less(j, s + a, s + b, c1);
  below0 = group_sum<G>(below0);
  below1 = group_sum<G>(below1);
  *len = below1 - below0;
  *first = s + below0;
}

template <int VW>
__device__ inline void store_value(double *__restrict__ x, int64_t o, double re, double im) {
  if (VW == 1) x[o] = re;
  else *reinterpret_cast<double2 *>(x + 2 * o) = make_double2(re, im);  // 16-byte aligned: the buffer is, o counts pairs
}

template <int VW>
__device__ inline void move_value(const double *__restrict__ src, int64_t p, double *__restrict__ dst, int64_t o) {
  if (VW == 1) dst[o] = src[p];
  else *reinterpret_cast<double2 *>(dst + 2 * o) = *reinterpret_cast<const double2 *>(src + 2 * p);  // both 16-byte aligned
}

// The copy pass behind run_in_row: result row r is the run of Cp[r + 1] - Cp[r] entries that starts at source position
// first[r] (no second search), its indices moved down by `shift` (a window's first column; 0: as they are)
template <int G, int VW>
__global__ __launch_bounds__(kRowThreads) void run_copy_kernel(const int *__restrict__ Aj, const double *__restrict__ Ax,
                                                               const int64_t *__restrict__ first, int64_t nr, int shift,
                                                               const int64_t *__restrict__ Cp, int *__restrict__ Cj,
                                                               double *__restrict__ Cx) {
  constexpr int kGroups = kRowThreads / G;
  const int lane = threadIdx.x % G;
  int64_t r = (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  for (; r < nr; r += stride) {
    const int64_t o = Cp[r], p = first[r];
    const int n = (int)(Cp[r + 1] - o);
    for (int e = lane; e < n; e += G) {
      Cj[o + e] = Aj[p + e] - shift;
      move_value<VW>(Ax, p + e, Cx, o + e);
    }
  }
}

// ---- room for a result whose dimensions and value kind the caller set ------------------------------------------------
// nnz is known beforehand: pointers, indices and values
inline void allocate_result(Matrix *C, int64_t nnz) {
  C->nnz = nnz;
  C->rowptr64.alloc((size_t)C->nrows_local + 1);
  C->colidx.alloc((size_t)nnz);
  C->val.alloc((size_t)nnz * (size_t)C->vw);
}

// C's pointers are scanned: read nnz back (the one 8-byte read-back) and make room for indices and values
inline void allocate_entries(Matrix *C, hipStream_t s) {
  int64_t nnz = 0;
  SPL_HIP(hipMemcpyAsync(&nnz, C->rowptr64.get() + C->nrows_local, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  C->nnz = nnz;
  C->colidx.alloc((size_t)nnz);
  C->val.alloc((size_t)nnz * (size_t)C->vw);
}

inline void zero_pointers(Matrix *C, hipStream_t s) {
  SPL_HIP(hipMemsetAsync(C->rowptr64.get(), 0, ((size_t)C->nrows_local + 1) * sizeof(int64_t), s));
}

inline void empty_result(Matrix *C, hipStream_t s) {
  allocate_result(C, 0);
  zero_pointers(C, s);
}

}  // namespace spl

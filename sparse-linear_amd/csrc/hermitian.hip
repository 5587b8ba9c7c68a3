// hermitian.hip — `hermitian m = ctrans m == m` (Sparse.hs:377-379) on a device handle, under the derived Eq of
// Sparse.hs:78: dimensions, pointers, indices and values, the values with IEEE ==.
//
// The conjugate transpose is not built.  With strictly ascending indices, `ctrans m == m` holds iff the matrix is
// square and every stored entry (i, j, a) has a stored entry (j, i, b) with  re b == re a  and  im b == -im a
// (real values: b == a).  The map entry -> mirror is injective and both patterns have equally many entries, so
// "every entry has a mirror" already makes the two patterns equal, and with them the pointer and index arrays; the
// values then compare entry by entry, which is the same test read from the other side.
//
// Kernel: G lanes side by side take the entries of a row (G: the power of two at or above the mean row length),
// bisect row j's column indices for i and compare the two values.  A miss or a mismatch stores 0 to the one-word
// flag — every writer stores the same value, a plain vector store.  Nothing else is written.  What == gives for
// free: a NaN on either side is a mismatch; -0.0 equals +0.0; a diagonal entry is its own mirror, so it passes iff
// im == -im, i.e. im is a zero (and a real diagonal iff it is no NaN).
//
// Traffic: one stream of the image (4 bytes per row pointer, 4 + 8 vw bytes per entry), plus per entry
// ceil(log2 len(row j)) probes of 4 bytes into row j's indices — the rows a row points at are mostly the rows its
// neighbours point at, so these come from the caches — and one gather of 8 vw bytes.
#include "common.hpp"

namespace spl {
namespace {

typedef double double2v __attribute__((ext_vector_type(2)));

template <int VW>
struct Value;
template <>
struct Value<1> {
  typedef double type;
  static __device__ __forceinline__ bool mirrored(double a, double b) { return b == a; }
};
template <>
struct Value<2> {
  typedef double2v type;
  static __device__ __forceinline__ bool mirrored(double2v a, double2v b) { return b.x == a.x && b.y == -a.y; }
};

template <int VW, int G>
__global__ __launch_bounds__(256) void hermitian_kernel(int64_t n, const int *__restrict__ ptr,
                                                        const int *__restrict__ idx,
                                                        const typename Value<VW>::type *__restrict__ val,
                                                        int *__restrict__ flag) {
  const int lane = threadIdx.x % G;
  const int64_t rows_per_pass = (int64_t)gridDim.x * (256 / G);
  for (int64_t i = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; i < n; i += rows_per_pass) {
    const int end = ptr[i + 1];
    for (int p = ptr[i] + lane; p < end; p += G) {
      const int j = idx[p];  // < ncols == n: row j exists
      int q = p;             // a diagonal entry is its own mirror
      bool found = true;
      if (j != i) {
        int lo = ptr[j];
        const int hi_end = ptr[j + 1];
        int hi = hi_end;
        while (lo < hi) {
          const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
          if (idx[mid] < i) lo = mid + 1; else hi = mid;
        }
        found = lo < hi_end && idx[lo] == i;
        q = lo;
      }
      if (!found || !Value<VW>::mirrored(val[p], val[q])) *flag = 0;
    }
  }
}

template <int VW, int G>
void launch(const Matrix *m, int *flag, hipStream_t s) {
  const int64_t n = m->nrows_local;
  int64_t blocks = (n + (256 / G) - 1) / (256 / G);
  if (blocks > 256 * 64) blocks = 256 * 64;  // the rest by the grid-stride loop
  hipLaunchKernelGGL((hermitian_kernel<VW, G>), dim3((unsigned)blocks), dim3(256), 0, s, n, m->rowptr.get(),
                     m->colidx.get(), reinterpret_cast<const typename Value<VW>::type *>(m->val.get()), flag);
}

template <int VW>
void launch_for_mean(const Matrix *m, int *flag, hipStream_t s) {
  const int64_t mean = (m->nnz + m->nrows_local - 1) / m->nrows_local;
  if (mean <= 4) launch<VW, 4>(m, flag, s);
  else if (mean <= 8) launch<VW, 8>(m, flag, s);
  else if (mean <= 16) launch<VW, 16>(m, flag, s);
  else if (mean <= 32) launch<VW, 32>(m, flag, s);
  else launch<VW, 64>(m, flag, s);
}

}  // namespace

// m: a whole handle with 32-bit row pointers (the caller has checked both)
int hermitian_device(const Matrix *m, hipStream_t s) {
  if (m->nrows_global != m->ncols) return 0;  // the dimensions differ: False, no error (Sparse.hs:78)
  if (m->nnz == 0 || m->nrows_local == 0) return 1;
  DBuf<int> flag(1);
  SPL_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(flag.get()), 1, 1, s));
  if (m->vw == 2) launch_for_mean<2>(m, flag.get(), s); else launch_for_mean<1>(m, flag.get(), s);
  SPL_HIP(hipGetLastError());
  int h = 0;
  SPL_HIP(hipMemcpyAsync(&h, flag.get(), sizeof(int), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  return h ? 1 : 0;
}

}  // namespace spl

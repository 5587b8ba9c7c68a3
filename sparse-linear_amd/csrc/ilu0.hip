// ilu0.hip — the incomplete LU factorisation without fill, ILU(0), on device handles, Double and packed Complex Double:
// the producer of what the sparse triangular solves (trisolve.hip) apply.  L (unit lower) and U share one handle with
// A's own pattern, so the result goes to spl_trisolve_analyze as it is (lower + unit diagonal, upper + stored diagonal).
//
// Arithmetic contract (include/sparse_linear_hip.h): the serial IKJ loop on a copy of A's values,
//     for i:  for each stored (i,k), k < i, ascending:   a_ik = a_ik / u_kk;
//                 for each stored (i,j), j > k, ascending:   if (k,j) is stored:  a_ij = a_ij - a_ik * a_kj
// with every real operation separately rounded (-ffp-contract=off), the IEEE division (no stored reciprocal) and, on
// complex handles, Data.Complex's product and scaled quotient: the mul / sub / quot of tri_arith.hpp.  Every entry
// (i,j) receives its updates in ascending k, each update one product and one difference, so the result depends on
// neither the level schedule nor the lanes per row nor any launch shape: it is the serial loop bit for bit.
//
// One row is worked by a group of G lanes; the steps k run one after the other.  Entry t of a row is only ever read and
// written by lane (t - row_start) % G, and a_ik reaches the other lanes of the group by a shuffle from its owner, never
// through memory: inside a row no memory ordering is needed.  Across rows, row k and u_kk are final before row i
// starts, by the two mechanisms of trisolve.hip and no other: launch order on the stream (one launch per WIDE level)
// and __syncthreads() between the levels ONE workgroup walks (NARROW).  No kernel waits for another workgroup: no
// flags, no polled counters, no grid barrier, no cooperative launch, no floating-point atomic.  The values array is
// read with plain loads (no __restrict__): it is written in the same kernel.
//
// Schedule (tri_levels.hpp): row i waits for the rows k < i of its lower pattern, which is the dependency structure of
// the lower triangular solve; the level tables and the wide / narrow plan are those of the solves.  The plan object
// holds the pattern, the diagonal positions and the level tables, no values and no scratch: one plan factors real and
// complex handles alike, and several host threads may factor on it at once.
#include <math.h>

#include "row_groups.hpp"
#include "tri_arith.hpp"
#include "tri_levels.hpp"

namespace spl {

namespace {

// The analysed pattern in device memory; rows in their original places, reached through the level order
struct IluView {
  const int *rows;       // n: the row at every position of the level order
  const int *ptr;        // n + 1
  const int *col;        // nnz, ascending inside a row
  const int *diag;       // n: position of the stored a_ii, -1 when row i stores none
  const int *upper;      // n: first position of row i with a column above i (ptr[i + 1] when there is none)
  const int *level_ptr;  // levels + 1
};

// Row i = rows[p] by the G lanes of its group; every lane of the group is here and runs the same trips
template <int G, int VW>
__device__ inline void factor_row(const IluView &P, double *val, int p, int lane) {
  typedef Val<VW> V;
  const int i = P.rows[p];
  const int s = P.ptr[i], e = P.ptr[i + 1];
  const int di = P.diag[i];
  const int lower_end = di >= 0 ? di : P.upper[i];  // the entries (i,k) with k < i are [s, lower_end)
  for (int q = s; q < lower_end; ++q) {             // step k = col[q]
    const int k = P.col[q];
    const int owner = (q - s) & (G - 1);
    V a = V();
    if (lane == owner) a = load_val<VW>(val, q);  // its current value: the owner wrote every update of it
    a = from_lane<G>(a, owner);
    const int dk = P.diag[k];
    V u = V();  // a row without a stored diagonal: u_kk = 0, and IEEE says what the quotient is
    if (dk >= 0) u = load_val<VW>(val, dk);
    const V l = quot(a, u);
    if (lane == owner) store_val(val, q, l);
    const int ks = P.upper[k], ke = P.ptr[k + 1];  // the entries (k,j) with j > k
    // the entries behind q in chunks of G: this lane takes those it owns
    for (int t = q + 1 + ((lane - (q + 1 - s)) & (G - 1)); t < e; t += G) {
      const int j = P.col[t];
      const int r = ks + count_less(P.col, ks, ke, j);
      if (r < ke && P.col[r] == j) store_val(val, t, sub(load_val<VW>(val, t), mul(l, load_val<VW>(val, r))));
    }
  }
}

// WIDE: positions [row0, row1) are one level
template <int G, int VW>
__global__ __launch_bounds__(kRowThreads) void ilu0_wide_kernel(IluView P, double *val, int row0, int row1) {
  constexpr int kGroups = kRowThreads / G;
  const int lane = threadIdx.x % G;
  int64_t p = (int64_t)row0 + (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  for (; p < row1; p += stride) factor_row<G, VW>(P, val, (int)p, lane);
}

// NARROW: ONE workgroup walks the levels [level0, level1); every thread of it reaches every barrier
template <int G, int VW>
__global__ __launch_bounds__(kRowThreads) void ilu0_narrow_kernel(IluView P, double *val, int level0, int level1) {
  constexpr int kGroups = kRowThreads / G;
  const int lane = threadIdx.x % G;
  const int group = threadIdx.x / G;
  for (int l = level0; l < level1; ++l) {
    const int r0 = P.level_ptr[l], r1 = P.level_ptr[l + 1];
    for (int p = r0 + group; p < r1; p += kGroups) factor_row<G, VW>(P, val, p, lane);
    __syncthreads();  // the level's rows are final before the next level reads them
  }
}

// differing row pointers and columns of two patterns of equal n and nnz: an integer count
__global__ __launch_bounds__(kRowThreads) void ilu0_compare_kernel(const int *__restrict__ ptr_a,
                                                                   const int *__restrict__ ptr_b, int64_t nptr,
                                                                   const int *__restrict__ col_a,
                                                                   const int *__restrict__ col_b, int64_t nnz,
                                                                   unsigned long long *__restrict__ count) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  int mine = 0;
  for (int64_t q = i; q < nptr; q += stride) mine += ptr_a[q] != ptr_b[q];
  for (int64_t q = i; q < nnz; q += stride) mine += col_a[q] != col_b[q];
  if (mine) atomicAdd(count, (unsigned long long)mine);
}

// rows whose stored u_ii is exactly zero (both parts, when complex): an integer count
template <int VW>
__global__ __launch_bounds__(kRowThreads) void ilu0_zero_pivot_kernel(const int *__restrict__ diag, const double *val,
                                                                      int64_t n, unsigned long long *__restrict__ count) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  int mine = 0;
  for (; i < n; i += stride) {
    const int d = diag[i];
    if (d < 0) continue;  // counted by the analysis
    if (VW == 1) mine += val[d] == 0.0;
    else mine += val[2 * (int64_t)d] == 0.0 && val[2 * (int64_t)d + 1] == 0.0;
  }
  if (mine) atomicAdd(count, (unsigned long long)mine);
}

template <typename T>
void upload_ints(DBuf<T> &dst, const std::vector<T> &src, hipStream_t s, size_t *bytes) {
  dst.alloc(src.size());
  if (!src.empty()) SPL_HIP(hipMemcpyAsync(dst.get(), src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, s));
  *bytes += (src.size() ? src.size() : 1) * sizeof(T);
}

}  // namespace

struct IluPlan : ObjectHead {  // no values: vw stays 1
  IluPlan() : ObjectHead(kIluMagic) {}
  int64_t nnz = 0, missing = 0, longest = 0;
  int nlevels = 0;
  std::vector<tri::Segment> segments;  // host: the launch plan
  DBuf<int> rows, ptr, col, diag, upper, level_ptr;
  size_t bytes = 0;
  std::atomic<int64_t> factorisations{0};
  IluView view() const { return IluView{rows.get(), ptr.get(), col.get(), diag.get(), upper.get(), level_ptr.get()}; }
};

// A is whole, square, with 32-bit row pointers: checked by the caller.  Synchronises.
int ilu0_analyze(const Matrix *A, IluPlan **out) {
  hipStream_t s = nullptr;
  std::unique_ptr<IluPlan> P(new IluPlan);
  P->device = A->device;
  P->n = (int)A->nrows_local;
  P->nnz = A->nnz;
  const int n = (int)P->n;
  // the pattern, once
  std::vector<int> rowptr((size_t)n + 1, 0), colidx((size_t)A->nnz);
  if (n > 0) SPL_HIP(hipMemcpyAsync(rowptr.data(), A->rowptr.get(), ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
  if (A->nnz > 0)
    SPL_HIP(hipMemcpyAsync(colidx.data(), A->colidx.get(), (size_t)A->nnz * sizeof(int), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  tri::Triangle tr;
  tri::take_triangle(n, rowptr.data(), colidx.data(), true, tr);
  std::vector<int> upper((size_t)n);
  for (int i = 0; i < n; ++i) {
    const int below = tr.off_ptr[i + 1] - tr.off_ptr[i];
    upper[i] = rowptr[i] + below + (tr.diag_src[i] >= 0 ? 1 : 0);
    if (tr.diag_src[i] < 0) P->missing++;
    const int64_t len = rowptr[i + 1] - rowptr[i];
    if (len > P->longest) P->longest = len;
  }
  std::vector<int> level;
  const int nlevels = tri::levels(n, tr.off_ptr.data(), tr.off_col.data(), true, level);
  tri::Plan plan;
  tri::plan(n, rowptr.data(), level, nlevels, tri::read_knobs(), plan);  // the FULL rows: G follows whole rows
  P->nlevels = nlevels;
  P->segments = plan.segments;
  upload_ints(P->rows, plan.rows, s, &P->bytes);
  upload_ints(P->ptr, rowptr, s, &P->bytes);
  upload_ints(P->col, colidx, s, &P->bytes);
  upload_ints(P->diag, tr.diag_src, s, &P->bytes);
  upload_ints(P->upper, upper, s, &P->bytes);
  upload_ints(P->level_ptr, plan.level_ptr, s, &P->bytes);
  SPL_HIP(hipStreamSynchronize(s));  // the host vectors go on return
  *out = P.release();
  return SPL_OK;
}

namespace {

template <int G, int VW>
void launch_ilu_segment(const tri::Segment &seg, const IluView &view, double *val, hipStream_t s) {
  if (seg.kind == tri::kWide)
    hipLaunchKernelGGL((ilu0_wide_kernel<G, VW>), dim3(grid_rows(seg.row1 - seg.row0, G)), dim3(kRowThreads), 0, s, view,
                       val, seg.row0, seg.row1);
  else
    hipLaunchKernelGGL((ilu0_narrow_kernel<G, VW>), dim3(1), dim3(kRowThreads), 0, s, view, val, seg.level0, seg.level1);
}

unsigned long long read_count(const DBuf<unsigned long long> &count, hipStream_t s) {
  unsigned long long h = 0;
  SPL_HIP(hipMemcpyAsync(&h, count.get(), sizeof(h), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  return h;
}

}  // namespace

// A: whole, 32-bit row pointers, on the plan's device (checked by the caller); C's dimensions and value kind are set by
// the caller.  SPL_ERROR_invalid_matrix when A's pattern is not the analysed one (C is left empty), else C receives
// A's pattern and the L\U values: SPL_OK or SPL_WARNING_singular_matrix.  Synchronises s.
int ilu0_factor(IluPlan *P, const Matrix *A, Matrix *C, hipStream_t s) {
  const int64_t n = P->n, nnz = P->nnz;
  if (A->nrows_local != n || A->ncols != n || A->nnz != nnz) return SPL_ERROR_invalid_matrix;
  DBuf<unsigned long long> count(1);
  SPL_HIP(hipMemsetAsync(count.get(), 0, sizeof(unsigned long long), s));
  if (n > 0) {
    const int64_t most = n + 1 > nnz ? n + 1 : nnz;
    hipLaunchKernelGGL(ilu0_compare_kernel, dim3(grid_flat(most, 1024)), dim3(kRowThreads), 0, s, P->ptr.get(),
                       A->rowptr.get(), n + 1, P->col.get(), A->colidx.get(), nnz, count.get());
    SPL_HIP(hipGetLastError());
    if (read_count(count, s) != 0) return SPL_ERROR_invalid_matrix;
  }
  const int vw = A->vw;
  allocate_result(C, nnz);
  SPL_HIP(hipMemcpyAsync(C->rowptr64.get(), A->rowptr64.get(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
  if (nnz > 0) {
    SPL_HIP(hipMemcpyAsync(C->colidx.get(), A->colidx.get(), (size_t)nnz * sizeof(int), hipMemcpyDeviceToDevice, s));
    SPL_HIP(hipMemcpyAsync(C->val.get(), A->val.get(), (size_t)nnz * (size_t)vw * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  const IluView view = P->view();
  double *val = C->val.get();
  for (const tri::Segment &seg : P->segments) {
    for_group_and_width(seg.group, vw, [&](auto g, auto w) {
      launch_ilu_segment<decltype(g)::value, decltype(w)::value>(seg, view, val, s);
    });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      set_last_error("ilu0 launch", e);
      (void)hipStreamSynchronize(s);
      return SPL_ERROR_device;
    }
  }
  unsigned long long zero = 0;
  if (n > 0) {  // the count is still 0: the patterns agreed
    if (vw == 1)
      hipLaunchKernelGGL((ilu0_zero_pivot_kernel<1>), dim3(grid_flat(n, 1024)), dim3(kRowThreads), 0, s, P->diag.get(), val,
                         n, count.get());
    else
      hipLaunchKernelGGL((ilu0_zero_pivot_kernel<2>), dim3(grid_flat(n, 1024)), dim3(kRowThreads), 0, s, P->diag.get(), val,
                         n, count.get());
    SPL_HIP(hipGetLastError());
    zero = read_count(count, s);
  } else {
    SPL_HIP(hipStreamSynchronize(s));
  }
  P->factorisations.fetch_add(1, std::memory_order_relaxed);
  return (zero > 0 || P->missing > 0) ? SPL_WARNING_singular_matrix : SPL_OK;
}

void ilu0_info(const IluPlan *P, int64_t info[8]) {
  info[0] = P->n;
  info[1] = P->nnz;
  info[2] = P->nlevels;
  info[3] = (int64_t)P->segments.size();
  info[4] = P->missing;
  info[5] = P->longest;
  info[6] = (int64_t)P->bytes;
  info[7] = P->factorisations.load(std::memory_order_relaxed);
}

void ilu0_delete(IluPlan *P) { delete_object(P); }

}  // namespace spl

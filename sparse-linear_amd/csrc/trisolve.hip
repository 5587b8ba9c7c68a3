// trisolve.hip — sparse triangular solves on device handles, Double and packed Complex Double, k right-hand sides:
//   T x = b,  T^T x = b,  T^H x = b,   T the lower or upper triangle of a whole square handle.
//
// Arithmetic contract (include/sparse_linear_hip.h): row i computes  acc = b_i;  acc = acc - t_ij * x_j  over the
// stored off-diagonal entries of the row in ascending column order;  x_i = acc / d_i  (unit diagonal: x_i = acc).
// Every real operation is separately rounded (-ffp-contract=off), the division is the IEEE division, the complex
// product is Data.Complex's and the complex quotient its scaled form.  There is no tree sum inside a row: the lanes of
// a group gather x_j and form the products of G entries side by side, and the products are then folded into the
// accumulator one after the other in column order (a shuffle per product, the same in every lane of the group).  The
// result therefore does not depend on the schedule, the group width, the number of right-hand sides or the launch
// shapes: it is the serial loop bit for bit.
//
// Schedule (tri_levels.hpp).  The analysis downloads the pattern once, computes the level of every row on the host and
// stores a copy of the triangle whose rows are permuted so that a level is contiguous (off-diagonal entries and the
// diagonal apart).  A level of many rows is one launch of the row-groups frame (WIDE); a run of small levels is one
// launch of a single workgroup that walks them with __syncthreads() between two levels (NARROW).  No kernel here waits
// for another workgroup: no flags, no counters polled in a loop, no grid barrier, no cooperative launch, no
// floating-point atomic.  Dependencies are kept by launch order on the stream and by the workgroup barrier alone.
//
// B and X may be the same array (in place): row i reads b_i before it writes x_i and nobody else reads either, and
// every x_j a row gathers was written by an earlier launch or before an earlier barrier.  Hence no __restrict__ on them.
#include <math.h>

#include <mutex>

#include "row_groups.hpp"
#include "tri_arith.hpp"
#include "tri_levels.hpp"

namespace spl {

namespace {

constexpr int kTriGroupCols = 8;  // right-hand sides one pass of the launch chain takes (kSolveGroup of the LU solves)

// values and their arithmetic (Val, load_val / store_val, mul / sub / quot, from_lane): tri_arith.hpp

// The permuted image of one triangle, in device memory
struct ImageView {
  const int *rows;      // n: original row of every position
  const int *ptr;       // n + 1: off-diagonal entries of every position
  const int *col;       // original column of every entry
  const double *val;    // VW doubles per entry
  const double *diag;   // VW doubles per position; not read with a unit diagonal
  const int *level_ptr; // levels + 1
  int unit;
};

// One row by the G lanes of its group; every lane of the group is here and runs the same trips.  KC accumulators side
// by side: column c < kc of the pass, a column past kc - 1 repeats column kc - 1 (read again, never stored).
template <int G, int VW, int KC>
__device__ inline void solve_row(const ImageView &T, int p, int lane, const double *B, int64_t ldb, double *X,
                                 int64_t ldx, int kc) {
  typedef Val<VW> V;
  const int64_t i = T.rows[p];
  const int s = T.ptr[p], e = T.ptr[p + 1];
  V acc[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    const int cc = c < kc ? c : kc - 1;
    acc[c] = load_val<VW>(B, i + (int64_t)cc * ldb);
  }
  for (int base = s; base < e; base += G) {
    const int q = base + lane < e ? base + lane : e - 1;  // a lane past the row repeats its last entry, never folded
    const int64_t j = T.col[q];
    const V t = load_val<VW>(T.val, q);
    V prod[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      const int cc = c < kc ? c : kc - 1;
      prod[c] = mul(t, load_val<VW>(X, j + (int64_t)cc * ldx));
    }
    const int cnt = e - base < G ? e - base : G;
    for (int l = 0; l < cnt; ++l) {  // the fold: in column order, one product after the other
#pragma unroll
      for (int c = 0; c < KC; ++c) acc[c] = sub(acc[c], from_lane<G>(prod[c], l));
    }
  }
  if (!T.unit) {
    const V d = load_val<VW>(T.diag, p);
#pragma unroll
    for (int c = 0; c < KC; ++c) acc[c] = quot(acc[c], d);
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < KC; ++c)
      if (c < kc) store_val(X, i + (int64_t)c * ldx, acc[c]);
  }
}

// WIDE: positions [row0, row1) are one level
template <int G, int VW, int KC>
__global__ __launch_bounds__(kRowThreads) void tri_wide_kernel(ImageView T, int row0, int row1, const double *B,
                                                               int64_t ldb, double *X, int64_t ldx, int kc) {
  constexpr int kGroups = kRowThreads / G;
  const int lane = threadIdx.x % G;
  int64_t p = (int64_t)row0 + (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  for (; p < row1; p += stride) solve_row<G, VW, KC>(T, (int)p, lane, B, ldb, X, ldx, kc);
}

// NARROW: ONE workgroup walks the levels [level0, level1); every thread of it reaches every barrier
template <int G, int VW, int KC>
__global__ __launch_bounds__(kRowThreads) void tri_narrow_kernel(ImageView T, int level0, int level1, const double *B,
                                                                 int64_t ldb, double *X, int64_t ldx, int kc) {
  constexpr int kGroups = kRowThreads / G;
  const int lane = threadIdx.x % G;
  const int group = threadIdx.x / G;
  for (int l = level0; l < level1; ++l) {
    const int r0 = T.level_ptr[l], r1 = T.level_ptr[l + 1];
    for (int p = r0 + group; p < r1; p += kGroups) solve_row<G, VW, KC>(T, p, lane, B, ldb, X, ldx, kc);
    __syncthreads();  // the level's x is written before the next level gathers it
  }
}

// ---- building an image: values gathered on the device, the pattern comes from the host -----------------------------
template <int VW>
__global__ __launch_bounds__(kRowThreads) void tri_gather_kernel(const double *__restrict__ from,
                                                                 const int *__restrict__ src, int64_t n, int conj,
                                                                 double *__restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; i < n; i += stride) {
    const int q = src[i];
    if (VW == 1) {
      out[i] = q < 0 ? 0.0 : from[q];
    } else {
      double2 z = make_double2(0.0, 0.0);
      if (q >= 0) z = *reinterpret_cast<const double2 *>(from + 2 * (int64_t)q);
      if (conj) z.y = -z.y;
      *reinterpret_cast<double2 *>(out + 2 * i) = z;
    }
  }
}

// rows whose d_i is missing or zero (both parts, when complex): an integer count
template <int VW>
__global__ __launch_bounds__(kRowThreads) void tri_zero_diag_kernel(const double *__restrict__ diag, int64_t n,
                                                                    unsigned long long *__restrict__ count) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  int mine = 0;
  for (; i < n; i += stride) {
    if (VW == 1) mine += diag[i] == 0.0;
    else mine += diag[2 * i] == 0.0 && diag[2 * i + 1] == 0.0;
  }
  if (mine) atomicAdd(count, (unsigned long long)mine);
}

struct TriImage {
  DBuf<int> rows, ptr, col, level_ptr;
  DBuf<double> val, diag;
  tri::Plan plan;  // host: the segments
  size_t bytes = 0;
  ImageView view(int unit) const {
    return ImageView{rows.get(), ptr.get(), col.get(), val.get(), diag.get(), level_ptr.get(), unit};
  }
};

template <typename T>
void upload_vec(DBuf<T> &dst, const std::vector<T> &src, hipStream_t s, size_t *bytes) {
  dst.alloc(src.size());
  if (!src.empty()) SPL_HIP(hipMemcpyAsync(dst.get(), src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, s));
  *bytes += (src.size() ? src.size() : 1) * sizeof(T);
}

// An image from an off-diagonal pattern in original row order (ptr / col / src) and the diagonal's sources: levels,
// plan, permuted arrays up, values gathered from `from_off` / `from_diag` (conjugated when conj).  Synchronises s.
void build_image(TriImage &img, int n, int vw, bool lower, bool unit, const tri::Knobs &knobs, const std::vector<int> &ptr,
                 const std::vector<int> &col, const std::vector<int> &src, const std::vector<int> &diag_src,
                 const double *from_off, const double *from_diag, bool conj, hipStream_t s) {
  std::vector<int> level;
  const int nlevels = tri::levels(n, ptr.data(), col.data(), lower, level);
  tri::plan(n, ptr.data(), level, nlevels, knobs, img.plan);
  std::vector<int> pptr, pcol, psrc, pdiag((size_t)n);
  tri::permute_rows(n, ptr.data(), col.data(), src.data(), img.plan, pptr, pcol, psrc);
  for (int p = 0; p < n; ++p) pdiag[p] = diag_src[img.plan.rows[p]];
  img.bytes = 0;
  upload_vec(img.rows, img.plan.rows, s, &img.bytes);
  upload_vec(img.ptr, pptr, s, &img.bytes);
  upload_vec(img.col, pcol, s, &img.bytes);
  upload_vec(img.level_ptr, img.plan.level_ptr, s, &img.bytes);
  const int64_t nnz = (int64_t)pcol.size();
  img.val.alloc((size_t)nnz * (size_t)vw);
  img.bytes += (size_t)(nnz ? nnz : 1) * (size_t)vw * sizeof(double);
  DBuf<int> d_src, d_dsrc;
  size_t scratch = 0;
  upload_vec(d_src, psrc, s, &scratch);
  auto gather = [&](const double *from, const int *idx, int64_t count, double *out) {
    if (count == 0) return;
    if (vw == 1)
      hipLaunchKernelGGL((tri_gather_kernel<1>), dim3(grid_flat(count)), dim3(kRowThreads), 0, s, from, idx, count, 0, out);
    else
      hipLaunchKernelGGL((tri_gather_kernel<2>), dim3(grid_flat(count)), dim3(kRowThreads), 0, s, from, idx, count,
                         conj ? 1 : 0, out);
    SPL_HIP(hipGetLastError());
  };
  gather(from_off, d_src.get(), nnz, img.val.get());
  if (!unit) {
    img.diag.alloc((size_t)n * (size_t)vw);
    img.bytes += (size_t)(n ? n : 1) * (size_t)vw * sizeof(double);
    upload_vec(d_dsrc, pdiag, s, &scratch);
    gather(from_diag, d_dsrc.get(), n, img.diag.get());
  }
  SPL_HIP(hipStreamSynchronize(s));  // the index scratch is released on return
}

}  // namespace

struct TriSolver : ObjectHead {
  bool upper = false, unit = false;
  tri::Knobs knobs;
  int64_t stored = 0, longest = 0, zero_diag = 0;
  TriImage img[3];                 // SPL_OP_n, _t, _h; real: _h is _t's
  std::atomic<bool> built[3];
  std::mutex lock;                 // the lazy build of the transposed images
  TriSolver() : ObjectHead(kTriMagic) { for (auto &b : built) b.store(false); }
};

// A is whole, square, with 32-bit row pointers: checked by the caller.  Returns SPL_OK or SPL_WARNING_singular_matrix.
int trisolve_analyze(const Matrix *A, int uplo, int diag, TriSolver **out) {
  hipStream_t s = nullptr;
  std::unique_ptr<TriSolver> T(new TriSolver);
  T->device = A->device;
  T->n = (int)A->nrows_local;
  T->vw = A->vw;
  T->upper = uplo == SPL_TRI_upper;
  T->unit = diag == SPL_DIAG_unit;
  T->knobs = tri::read_knobs();
  const int n = (int)T->n;
  // the pattern, once
  std::vector<int> rowptr((size_t)n + 1, 0), colidx((size_t)A->nnz);
  if (n > 0) SPL_HIP(hipMemcpyAsync(rowptr.data(), A->rowptr.get(), ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
  if (A->nnz > 0)
    SPL_HIP(hipMemcpyAsync(colidx.data(), A->colidx.get(), (size_t)A->nnz * sizeof(int), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  tri::Triangle tr;
  tri::take_triangle(n, rowptr.data(), colidx.data(), !T->upper, tr);
  T->stored = tr.stored;
  T->longest = tr.longest;
  build_image(T->img[0], n, T->vw, !T->upper, T->unit, T->knobs, tr.off_ptr, tr.off_col, tr.off_src, tr.diag_src,
              A->val.get(), A->val.get(), false, s);
  if (n > 0 && !T->unit) {  // a unit diagonal has d_i = 1: nothing to count
    DBuf<unsigned long long> count(1);
    SPL_HIP(hipMemsetAsync(count.get(), 0, sizeof(unsigned long long), s));
    if (T->vw == 1)
      hipLaunchKernelGGL((tri_zero_diag_kernel<1>), dim3(grid_flat(n, 1024)), dim3(kRowThreads), 0, s,
                         T->img[0].diag.get(), (int64_t)n, count.get());
    else
      hipLaunchKernelGGL((tri_zero_diag_kernel<2>), dim3(grid_flat(n, 1024)), dim3(kRowThreads), 0, s,
                         T->img[0].diag.get(), (int64_t)n, count.get());
    SPL_HIP(hipGetLastError());
    unsigned long long h = 0;
    SPL_HIP(hipMemcpyAsync(&h, count.get(), sizeof(h), hipMemcpyDeviceToHost, s));
    SPL_HIP(hipStreamSynchronize(s));
    T->zero_diag = (int64_t)h;
  }
  T->built[0].store(true, std::memory_order_release);
  const bool singular = T->zero_diag > 0;
  *out = T.release();
  return singular ? SPL_WARNING_singular_matrix : SPL_OK;
}

namespace {

// the transposed (conj: conjugated) image from the first one; the caller holds the lock.  Synchronises.
void build_transposed(TriSolver *T, int slot, bool conj) {
  hipStream_t s = nullptr;
  const TriImage &N = T->img[0];
  const int n = (int)T->n;
  std::vector<int> pptr((size_t)n + 1, 0);
  if (n > 0) SPL_HIP(hipMemcpyAsync(pptr.data(), N.ptr.get(), ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  std::vector<int> pcol((size_t)pptr[n]);
  if (!pcol.empty())
    SPL_HIP(hipMemcpyAsync(pcol.data(), N.col.get(), pcol.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  std::vector<int> tptr, tcol, tsrc;
  tri::transpose_image(n, pptr, pcol, N.plan, tptr, tcol, tsrc);
  // d of the transposed row j is d_j: its place in the first image's diagonal is j's position there
  build_image(T->img[slot], n, T->vw, T->upper /* the transpose of an upper triangle is a lower one */, T->unit, T->knobs,
              tptr, tcol, tsrc, N.plan.pos, N.val.get(), N.diag.get(), conj, s);
}

template <int G, int VW, int KC>
void launch_segment(const tri::Segment &seg, const ImageView &view, const double *B, int64_t ldb, double *X, int64_t ldx,
                    int kc, hipStream_t s) {
  if (seg.kind == tri::kWide)
    hipLaunchKernelGGL((tri_wide_kernel<G, VW, KC>), dim3(grid_rows(seg.row1 - seg.row0, G)), dim3(kRowThreads), 0, s,
                       view, seg.row0, seg.row1, B, ldb, X, ldx, kc);
  else
    hipLaunchKernelGGL((tri_narrow_kernel<G, VW, KC>), dim3(1), dim3(kRowThreads), 0, s, view, seg.level0, seg.level1, B,
                       ldb, X, ldx, kc);
}

}  // namespace

// arguments checked by the caller; enqueues on s.  The first transposed solve builds its image and synchronises.
int trisolve_solve(TriSolver *T, int op, int k, const double *d_B, int64_t ldb, double *d_X, int64_t ldx, hipStream_t s) {
  const int slot = op == SPL_OP_n ? 0 : (op == SPL_OP_h && T->vw == 2) ? 2 : 1;
  if (!T->built[slot].load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> hold(T->lock);
    if (!T->built[slot].load(std::memory_order_acquire)) {
      build_transposed(T, slot, slot == 2);
      T->built[slot].store(true, std::memory_order_release);
    }
  }
  const TriImage &img = T->img[slot];
  const ImageView view = img.view(T->unit ? 1 : 0);
  const int64_t vw = T->vw;
  for (int c0 = 0; c0 < k; c0 += kTriGroupCols) {
    const int kc = k - c0 < kTriGroupCols ? k - c0 : kTriGroupCols;
    const double *B = d_B + (int64_t)c0 * ldb * vw;
    double *X = d_X + (int64_t)c0 * ldx * vw;
    for (const tri::Segment &seg : img.plan.segments) {
      for_group_and_width(seg.group, T->vw, [&](auto g, auto w) {
        constexpr int G = decltype(g)::value, VW = decltype(w)::value;
        if (kc == 1) launch_segment<G, VW, 1>(seg, view, B, ldb, X, ldx, kc, s);
        else if (kc <= 4) launch_segment<G, VW, 4>(seg, view, B, ldb, X, ldx, kc, s);
        else launch_segment<G, VW, 8>(seg, view, B, ldb, X, ldx, kc, s);
      });
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) { set_last_error("trisolve launch", e); return SPL_ERROR_device; }
    }
  }
  return SPL_OK;
}

void trisolve_info(const TriSolver *T, int64_t info[8]) {
  info[0] = T->n;
  info[1] = T->stored;
  info[2] = T->img[0].plan.nlevels;
  info[3] = T->img[0].plan.launches();
  info[4] = T->zero_diag;
  info[5] = T->longest;
  size_t bytes = 0;
  int transposed = 0;
  for (int i = 0; i < 3; ++i)
    if (T->built[i].load(std::memory_order_acquire)) {
      bytes += T->img[i].bytes;
      if (i > 0) transposed = 1;
    }
  info[6] = (int64_t)bytes;
  info[7] = (T->vw == 2 ? 1 : 0) | (T->upper ? 2 : 0) | (T->unit ? 4 : 0) | (transposed ? 8 : 0);
}

void trisolve_delete(TriSolver *T) { delete_object(T); }

}  // namespace spl

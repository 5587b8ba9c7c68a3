// spmv_many.hip — CSR SpMV on k vectors at once, Double and packed Complex Double:
//   Y[:, j] = A X[:, j] (+ Y[:, j]),  j = 0 .. k-1,
// X and Y column-major (one vector after the other) with leading dimensions ldx, ldy counted in entries.
// This is what the reference does with one axpy_ per vector (Feast.hs:203-208 `multiplyWork`, Sparse.hs:482-488
// `mulM`); here A is streamed once per pass of up to kPass vectors instead of once per vector.
//
// Order contract (stronger than spmv_stream's): every (row, vector) accumulator folds  a * x + acc  over the row's
// stored entries in ascending column order, for rows of ANY length — there is no wavefront-tree shortcut for a row
// that covers a chunk, a lane simply carries its accumulators from one chunk to the next.  Every real operation is
// separately rounded (-ffp-contract=off), the complex product is Data.Complex's,
// (a :+ b) * (c :+ d) = (a*c - b*d) :+ (a*d + b*c), written as spmv_stream_z writes it.  Vector j's result is
// therefore the oracle's axpy_ / axpy_z on that column, bit for bit, always; and spl_matrix_spmv_dev's in
// SPL_ORDER_REFERENCE wherever that kernel keeps the order (rows within one chunk).  Always the CSR image: the
// handle's order setting and its blocked / SELL / panel images are not looked at.
//
// Structure (spmv_stream's): one wavefront owns 64 consecutive rows, whose entries [S, E) are contiguous; a chunk of
// 64 * EPL entries is loaded ONCE into registers (coalesced, non-temporal); then, for each tile of T vectors, the
// wavefront gathers x[c + j ldx], stages the products in its private LDS slice as [entry][vector of the tile] and
// lane l folds row l's entries of the chunk in order into T of its register accumulators.  No workgroup barrier:
// the LDS operations of one wavefront complete in issue order.  The XCD-aware block remap is spmv_stream's.
//
//            EPL  T  tiles  vectors/pass  LDS per workgroup   (VGPRs, occupancy: DESIGN.md §4.2)
//   Double    4   4   1-4      16           32 KiB
//   Complex   2   4   1-4      16           32 KiB
// k = 1 and k = 2 run with T = 1 and 2 (no work on vectors that are not there); k > 16 takes ceil(k / 16) passes
// over A.  k = 1 is spmv_stream without its 16-byte loads and without the long-row shortcut: expect it no faster
// than spl_matrix_spmv_dev, and slower on rows longer than a chunk, where correctness of the order is the point.
#include "common.hpp"

namespace spl {

namespace {

typedef double double2v __attribute__((ext_vector_type(2)));

constexpr int kWavesPerBlockMany = 4;
constexpr int kRowsPerBlockMany = kWavesPerBlockMany * 64;
constexpr int kPass = 16;  // vectors whose accumulators a lane keeps in registers during one pass over A

struct RealOps {
  typedef double V;
  static constexpr int EPL = 4;
  static __device__ inline V zero() { return 0.0; }
  static __device__ inline V mul(V a, V x) { return a * x; }
  static __device__ inline V add(V p, V acc) { return p + acc; }  // a * x + y
};

struct ComplexOps {
  typedef double2v V;
  static constexpr int EPL = 2;
  static __device__ inline V zero() {
    V z;
    z.x = 0.0;
    z.y = 0.0;
    return z;
  }
  static __device__ inline V mul(V a, V x) {  // (a :+ b) * (c :+ d) = (a*c - b*d) :+ (a*d + b*c)
    V p;
    p.x = a.x * x.x - a.y * x.y;
    p.y = a.x * x.y + a.y * x.x;
    return p;
  }
  static __device__ inline V add(V p, V acc) {  // a * x + y, componentwise
    V r;
    r.x = p.x + acc.x;
    r.y = p.y + acc.y;
    return r;
  }
};

// a value every lane holds alike, told to the compiler: chunk positions and their addresses then live in scalar registers
__device__ inline int64_t uniform64(int64_t v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(v & 0xffffffffLL));
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
  return (int64_t)(((unsigned long long)hi << 32) | lo);
}

// T: vectors per tile (staged together in LDS), NT: tiles per pass; (NT - 1) * T < kp <= T * NT vectors are live
template <typename Ops, int T, int NT, typename PtrT>
__global__ __launch_bounds__(kWavesPerBlockMany * 64, 4) void spmv_many_kernel(
    int64_t nrows, int64_t nblocks, const PtrT *__restrict__ rowptr, const int *__restrict__ colidx,
    const typename Ops::V *__restrict__ val, const typename Ops::V *__restrict__ X, int64_t ldx,
    typename Ops::V *__restrict__ Y, int64_t ldy, int kp, int accumulate) {
  typedef typename Ops::V V;
  constexpr int EPL = Ops::EPL;
  constexpr int CH = 64 * EPL;
  __shared__ V prod_all[kWavesPerBlockMany][CH * T];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t per_xcd = gridDim.x >> 3;  // XCD-aware remap as in spmv_stream (speed only)
  const int64_t rb = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  if (rb >= nblocks) return;
  const int64_t r0 = rb * kRowsPerBlockMany + (int64_t)wave * 64;
  if (r0 >= nrows) return;
  V *prod = prod_all[wave];
  const int64_t r = r0 + lane;
  const bool valid = r < nrows;
  const int64_t rc = valid ? r : nrows - 1;
  PtrT my_s = rowptr[rc];
  PtrT my_e = rowptr[rc + 1];
  const int nvalid = (nrows - r0) < 64 ? (int)(nrows - r0) : 64;
  const PtrT S = __shfl(my_s, 0, 64);
  const PtrT E = __shfl(my_e, nvalid - 1, 64);
  if (!valid) { my_s = E; my_e = E; }

  V acc[T * NT];
#pragma unroll
  for (int j = 0; j < T * NT; ++j) acc[j] = Ops::zero();
  if (accumulate && valid) {
#pragma unroll
    for (int j = 0; j < T * NT; ++j)
      if (j < kp) acc[j] = Y[r + (int64_t)j * ldy];
  }

  // (64-bit chunk positions whatever PtrT is: b0 + CH may pass 2^31 on the last chunk of a large matrix)
  const int64_t S64 = uniform64((int64_t)S), E64 = uniform64((int64_t)E);
  for (int64_t b0 = S64; b0 < E64; b0 += CH) {
    // ---- the chunk's entries, once for every vector of the pass
    // (an entry past E repeats entry E - 1 with the value 0 and is staged but never folded: no branch around
    // any load, so the loads of a chunk and the gathers of a tile are in flight together)
    int c[EPL];
    V a[EPL];
#pragma unroll
    for (int i = 0; i < EPL; ++i) {
      const int64_t k = b0 + (i * 64 + lane);
      const int64_t kc = k < E64 ? k : E64 - 1;
      c[i] = __builtin_nontemporal_load(colidx + kc);
      a[i] = __builtin_nontemporal_load(val + kc);
      if (k >= E64) a[i] = Ops::zero();
    }
    const int lo = (int)(((int64_t)my_s > b0 ? (int64_t)my_s : b0) - b0);
    const int64_t hi64 = ((int64_t)my_e < b0 + CH ? (int64_t)my_e : b0 + CH) - b0;
    const int hi = hi64 < 0 ? 0 : (int)hi64;  // a row that ended before this chunk
#pragma unroll
    for (int tile = 0; tile < NT; ++tile) {  // (NT - 1) * T < kp: every tile has a live vector
      // ---- gather, multiply, stage: [entry of the chunk][vector of the tile].  A vector past kp - 1 (last tile
      // only) repeats vector kp - 1 — a second read of the same address, never stored — which keeps conditions on
      // kp, and the copies of this loop the compiler would make for them, out of the chunk loop.
#pragma unroll
      for (int jt = 0; jt < T; ++jt) {
        const int j = tile * T + jt < kp ? tile * T + jt : kp - 1;
        const V *__restrict__ xj = X + (int64_t)j * ldx;
#pragma unroll
        for (int i = 0; i < EPL; ++i) {
          prod[(i * 64 + lane) * T + jt] = Ops::mul(a[i], xj[c[i]]);
        }
      }
      __builtin_amdgcn_wave_barrier();
      // ---- lane folds its row's slice of the chunk in order, T accumulators side by side
      for (int t = lo; t < hi; ++t) {
#pragma unroll
        for (int jt = 0; jt < T; ++jt) acc[tile * T + jt] = Ops::add(prod[t * T + jt], acc[tile * T + jt]);
      }
      __builtin_amdgcn_wave_barrier();
    }
  }
  if (valid) {
#pragma unroll
    for (int j = 0; j < T * NT; ++j)
      if (j < kp) Y[r + (int64_t)j * ldy] = acc[j];
  }
}

template <typename Ops, int T, int NT>
void launch_pass(const Matrix *m, int kp, const double *d_X, int64_t ldx, double *d_Y, int64_t ldy, int accumulate,
                 int64_t nblocks, unsigned grid, hipStream_t s) {
  typedef typename Ops::V V;
  const V *val = reinterpret_cast<const V *>(m->val.get());
  const V *X = reinterpret_cast<const V *>(d_X);
  V *Y = reinterpret_cast<V *>(d_Y);
  if (m->rowptr.get())
    hipLaunchKernelGGL((spmv_many_kernel<Ops, T, NT, int>), dim3(grid), dim3(kWavesPerBlockMany * 64), 0, s,
                       m->nrows_local, nblocks, m->rowptr.get(), m->colidx.get(), val, X, ldx, Y, ldy, kp, accumulate);
  else
    hipLaunchKernelGGL((spmv_many_kernel<Ops, T, NT, int64_t>), dim3(grid), dim3(kWavesPerBlockMany * 64), 0, s,
                       m->nrows_local, nblocks, m->rowptr64.get(), m->colidx.get(), val, X, ldx, Y, ldy, kp,
                       accumulate);
}

template <typename Ops>
int launch_passes(const Matrix *m, int k, const double *d_X, int64_t ldx, double *d_Y, int64_t ldy, int accumulate,
                  hipStream_t s) {
  const int64_t nblocks = (m->nrows_local + kRowsPerBlockMany - 1) / kRowsPerBlockMany;
  const int64_t grid64 = ((nblocks + 7) / 8) * 8;
  if (grid64 > 0x7fffffffLL) return SPL_ERROR_internal;
  const unsigned grid = (unsigned)grid64;
  const int64_t vw = m->vw;  // doubles per entry of X and Y
  for (int j0 = 0; j0 < k; j0 += kPass) {
    const int kp = k - j0 < kPass ? k - j0 : kPass;
    const double *x = d_X + (int64_t)j0 * ldx * vw;
    double *y = d_Y + (int64_t)j0 * ldy * vw;
    if (kp == 1) launch_pass<Ops, 1, 1>(m, kp, x, ldx, y, ldy, accumulate, nblocks, grid, s);
    else if (kp == 2) launch_pass<Ops, 2, 1>(m, kp, x, ldx, y, ldy, accumulate, nblocks, grid, s);
    else if (kp <= 4) launch_pass<Ops, 4, 1>(m, kp, x, ldx, y, ldy, accumulate, nblocks, grid, s);
    else if (kp <= 8) launch_pass<Ops, 4, 2>(m, kp, x, ldx, y, ldy, accumulate, nblocks, grid, s);
    else if (kp <= 12) launch_pass<Ops, 4, 3>(m, kp, x, ldx, y, ldy, accumulate, nblocks, grid, s);
    else launch_pass<Ops, 4, 4>(m, kp, x, ldx, y, ldy, accumulate, nblocks, grid, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { set_last_error("spmv_many launch", e); return SPL_ERROR_device; }
  }
  return SPL_OK;
}

// out (cols x rows, row-major) = transpose of in (rows x cols, row-major); one thread per entry of out
template <typename V>
__global__ __launch_bounds__(256) void transpose_dense_kernel(int64_t rows, int64_t cols, const V *__restrict__ in,
                                                              V *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * cols) return;
  const int64_t c = i / rows, r = i - c * rows;
  out[i] = in[r * cols + c];
}

}  // namespace

int launch_spmv_many(const Matrix *m, int k, const double *d_X, int64_t ldx, double *d_Y, int64_t ldy, int accumulate,
                     hipStream_t s) {
  if (m->nrows_local == 0 || k == 0) return SPL_OK;
  if (m->vw == 2) return launch_passes<ComplexOps>(m, k, d_X, ldx, d_Y, ldy, accumulate, s);
  return launch_passes<RealOps>(m, k, d_X, ldx, d_Y, ldy, accumulate, s);
}

int transpose_dense(int64_t rows, int64_t cols, int vw, const double *d_in, double *d_out, hipStream_t s) {
  const int64_t n = rows * cols;
  if (n == 0) return SPL_OK;
  const int64_t grid = (n + 255) / 256;
  if (grid > 0x7fffffffLL) return SPL_ERROR_internal;
  if (vw == 2)
    hipLaunchKernelGGL(transpose_dense_kernel<double2v>, dim3((unsigned)grid), dim3(256), 0, s, rows, cols,
                       reinterpret_cast<const double2v *>(d_in), reinterpret_cast<double2v *>(d_out));
  else
    hipLaunchKernelGGL(transpose_dense_kernel<double>, dim3((unsigned)grid), dim3(256), 0, s, rows, cols, d_in, d_out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_last_error("transpose_dense launch", e); return SPL_ERROR_device; }
  return SPL_OK;
}

}  // namespace spl

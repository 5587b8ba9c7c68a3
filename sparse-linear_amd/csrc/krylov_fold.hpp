// krylov_fold.hpp — the fixed-order fold and the value helpers shared by the Krylov solvers on device handles
// (krylov.hip: CG, BiCGSTAB and spl_vector_dot_dev; gmres.hip: restarted GMRES and spl_vector_dots_dev; eigsh.hip:
// thick-restart Lanczos; lobpcg.hip: LOBPCG; the last three through krylov_basis.hpp).  The arithmetic contract is the
// one at the head of krylov.hip: chunks of 4096 entries, 256 lanes that add their 16 entries in ascending order from
// +0.0, the halving tree, and the partials folded again by the same fold; the order is a function of the length alone.
// Device code and the host code that launches the levels; included by those files only.
#pragma once

#include <math.h>

#include <mutex>
#include <utility>

#include "row_groups.hpp"
#include "tri_arith.hpp"

namespace spl {

// Scratch of spl_vector_dot_dev and spl_vector_dots_dev: a block from the device pool PER CALL (krylov.hip).
struct DotBlock {
  DBuf<double> buf;
  hipEvent_t done = nullptr;  // behind the last kernel that reads or writes buf
  int device = 0;
  bool taken = false;         // a host thread is enqueueing on it
};
DotBlock *dot_block_take(int device, size_t doubles);
// the caller's kernels are enqueued on s (enqueued == false: a launch failed and s was synchronised)
void dot_block_give(DotBlock *b, hipStream_t s, bool enqueued);

namespace {

constexpr int kChunk = 4096;              // entries per chunk of the fold
constexpr int kLanes = 256;               // lanes of a chunk: the workgroup
constexpr int kSteps = kChunk / kLanes;   // 16 entries per lane
constexpr int kDefaultGrid = 2048;        // workgroups of a chunk kernel at most (SPL_KRYLOV_GRID)

// ---- values ----------------------------------------------------------------------------------------------------------
__device__ inline Val<1> add(Val<1> a, Val<1> b) { return Val<1>{a.re + b.re}; }
__device__ inline Val<2> add(Val<2> a, Val<2> b) { return Val<2>{a.re + b.re, a.im + b.im}; }
__device__ inline Val<1> conj_of(Val<1> a) { return a; }
__device__ inline Val<2> conj_of(Val<2> a) { return Val<2>{a.re, -a.im}; }
__device__ inline void accumulate(double *acc, Val<1> v) { acc[0] = acc[0] + v.re; }
__device__ inline void accumulate(double *acc, Val<2> v) {
  acc[0] = acc[0] + v.re;
  acc[1] = acc[1] + v.im;
}
__device__ inline bool is_zero(Val<1> a) { return a.re == 0.0; }
__device__ inline bool is_zero(Val<2> a) { return a.re == 0.0 && a.im == 0.0; }
__device__ inline bool is_finite(Val<1> a) { return isfinite(a.re); }
__device__ inline bool is_finite(Val<2> a) { return isfinite(a.re) && isfinite(a.im); }
template <int VW>
__device__ inline Val<VW> from_planes(const double *f, int dot);
template <>
__device__ inline Val<1> from_planes<1>(const double *f, int dot) {
  return Val<1>{f[dot]};
}
template <>
__device__ inline Val<2> from_planes<2>(const double *f, int dot) {
  return Val<2>{f[2 * dot], f[2 * dot + 1]};
}

// ---- the fold --------------------------------------------------------------------------------------------------------
// The 256 lane sums of NV planes to lane 0: s[t] += s[t + h], h = 128 ... 1.  Steps 128 and 64 through LDS in one
// expression per lane of the first wavefront, (s[t] + s[t + 128]) + (s[t + 64] + s[t + 192]); steps 32 ... 1 by
// shuffles inside that wavefront (lane t < h reads lane t + h, which the step before left final).  Every thread of the
// workgroup must be here.  lds: NV * 256 doubles.
template <int NV>
__device__ inline void lane_tree(double (&acc)[NV], double *lds) {
  const int t = threadIdx.x;
#pragma unroll
  for (int v = 0; v < NV; ++v) lds[v * kLanes + t] = acc[v];
  __syncthreads();
  if (t < 64) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const double *s = lds + v * kLanes;
      double a = (s[t] + s[t + 128]) + (s[t + 64] + s[t + 192]);
#pragma unroll
      for (int h = 32; h >= 1; h >>= 1) a = a + __shfl_down(a, h);
      acc[v] = a;
    }
  }
  __syncthreads();  // lds is written again for the workgroup's next chunk
}

// How a ONE-workgroup kernel behind the fold opens: the sum of the `count` partials of the last level, lane t taking
// t, t + 256, ... in ascending order from +0.0, then the tree.  Every thread of the workgroup must be here (the tree
// has barriers); lane 0 has the sum and goes on alone.
__device__ inline double sum_partials(const double *part, int count) {
  __shared__ double lds[kLanes];
  double f[1] = {0.0};
  for (int i = threadIdx.x; i < count; i += kLanes) f[0] = f[0] + part[i];
  lane_tree<1>(f, lds);
  return f[0];
}

// The chunks of [0, n) by the workgroups of the launch: body(i, acc) does the entry-wise work of entry i and adds its
// NV contributions to the lane's sums; part[v * stride + c] receives plane v of chunk c.
template <int NV, typename Body>
__device__ inline void chunk_partials(int64_t n, double *part, int64_t stride, Body body) {
  __shared__ double lds[NV * kLanes];
  const int t = threadIdx.x;
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    const int64_t base = c * kChunk + t;
#pragma unroll 4
    for (int k = 0; k < kSteps; ++k) {
      const int64_t i = base + (int64_t)k * kLanes;
      if (i < n) body(i, acc);
    }
    lane_tree<NV>(acc, lds);
    if (t == 0) {
#pragma unroll
      for (int v = 0; v < NV; ++v) part[v * stride + c] = acc[v];
    }
  }
}

// A level of the fold: plane blockIdx.y of `in` (count entries) to its ceil(count / 4096) partials.  stop: a flag of the
// caller's status block, or nullptr; the kernel returns without writing when it is set
__global__ __launch_bounds__(kLanes) void fold_kernel(const int *stop, int64_t count, const double *in, int64_t in_stride,
                                                      double *out, int64_t out_stride) {
  if (stop && *stop) return;
  const double *src = in + (int64_t)blockIdx.y * in_stride;
  chunk_partials<1>(count, out + (int64_t)blockIdx.y * out_stride, 0,
                    [&](int64_t i, double *acc) { acc[0] = acc[0] + src[i]; });
}

// ---- host: the levels of the fold -------------------------------------------------------------------------------------
inline int64_t chunks_of(int64_t n) { return (n + kChunk - 1) / kChunk; }

// doubles of scratch `planes` planes of the fold of n entries need: the first level and one middle level
inline size_t fold_scratch(int64_t n, int planes) {
  const int64_t c1 = chunks_of(n), c2 = chunks_of(c1);
  return (size_t)planes * (size_t)((c1 ? c1 : 1) + (c2 ? c2 : 1));
}

inline int chunk_grid_cap() {
  const char *e = getenv("SPL_KRYLOV_GRID");
  const long v = e ? atol(e) : 0;
  return v >= 1 && v <= 65535 ? (int)v : kDefaultGrid;
}

inline unsigned chunk_grid(int64_t n) {
  const int64_t c = chunks_of(n), cap = chunk_grid_cap();
  return (unsigned)(c < 1 ? 1 : c < cap ? c : cap);
}

// What the last level reads, and the middle levels that were launched before it
struct Partials {
  const double *p;
  int64_t stride;
  int count;
  int middle;
};

// The first level left chunks_of(n) partials per plane in `scratch` (stride chunks_of(n)); middle levels until at most
// 4096 are left.  The scratch is two parts (fold_scratch): planes * c1 entries for the first level, planes * c2 for the
// next, and the levels take turns between them: level k + 2 writes planes * c(k+2) <= planes * c(k) entries where level k
// wrote, so any number of levels fits.  One middle level serves up to 4096^3 entries; no vector in memory needs two.
inline Partials middle_levels(const int *stop, int64_t n, int planes, double *scratch, hipStream_t s) {
  int64_t count = chunks_of(n);
  const int64_t first_stride = count ? count : 1;
  double *cur = scratch, *other = scratch + (size_t)planes * (size_t)first_stride;
  int64_t stride = first_stride;
  int middle = 0;
  while (count > kChunk) {
    ++middle;
    const int64_t next = chunks_of(count);
    hipLaunchKernelGGL(fold_kernel, dim3(chunk_grid(count), planes), dim3(kLanes), 0, s, stop, count, cur, stride, other,
                       next);
    std::swap(cur, other);
    stride = next;
    count = next;
  }
  return Partials{cur, stride, (int)count, middle};
}

}  // namespace
}  // namespace spl

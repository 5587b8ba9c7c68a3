// amg.hip — aggregation AMG on device handles: the deterministic parallel aggregation of a handle's graph, the hierarchy
// built from it with the public handle operations, and the V-cycle that CG and BiCGSTAB (krylov.hip) take as their
// preconditioner.
//
// Aggregation (include/sparse_linear_hip.h): the graph and the priority are the colouring's (coloring.hip builds the
// transposed pattern for both).  The roots are the greedy maximal independent set of distance 2 in priority order,
// found in rounds.  A round is four launches over one thread per vertex:
//   1. best1[v] = the undecided vertex of v's closed neighbourhood N[v] that precedes the others (-1: none);
//   2. best2[v] = the one among best1[u], u in N[v], that precedes the others: the first undecided vertex within
//      distance <= 2 of v, whatever the vertices on the way are;
//   3. near[v]  = some u in N[v] is undecided with best2[u] == u, that is a root of this round;
//   4. an undecided v with best2[v] == v becomes a root; another one with near[u] set for some u in N[v] is out; the
//      others are counted and stay.
// Every launch reads what the launch before it finished and writes words of its own vertex only, so a round sees the
// state of its start and no kernel waits for another workgroup.  There is no floating-point operation; the integer
// atomics count vertices and aggregate sizes, sums and extremes that do not depend on their order.  The host issues
// SPL_AMG_CHECK_EVERY rounds and then looks at the counts: the rounds behind the last one find nobody undecided and
// change nothing, so neither that interval nor the grid (SPL_AMG_GRID) shows in any output.
//
// The cycle: x = w (.) b, x += w (.) (b - t) and r = b - t are one pass each over the large levels; the products with
// A, R and P are spl_matrix_spmv_dev's kernels in the reference order.  The tail levels (all of at most
// SPL_AMG_TAIL_ROWS rows and rows of at most 512 entries) run their whole sub-cycle, down and up, in ONE launch of ONE
// workgroup: a lane owns a row and walks it serially in ascending column order, which is the order of the
// launch-per-step path, the vectors are the object's work vectors, and workgroup barriers stand between the steps.
#include <limits.h>

#include <algorithm>
#include <mutex>

#include "row_groups.hpp"
#include "tri_arith.hpp"

namespace spl {

namespace {

constexpr int kAmgGridDefault = 2048;       // workgroups of an aggregation launch at most (SPL_AMG_GRID)
constexpr int kAmgCheckEveryDefault = 8, kAmgCheckEveryMax = 4096;
constexpr int kTailRowsMax = 1024;          // rows of a tail level at most: one lane a row (SPL_AMG_TAIL_ROWS)
constexpr int kTailThreads = 1024;
constexpr int kTailRowLen = 512;            // above it the SpMV of a row is no serial walk
constexpr int kVectorGrid = 4096;
constexpr int kWideRowsMax = 16384;         // a restriction of at most so many rows, of kWideRowsMean entries and more
constexpr int kWideRowsMean = 32;           // on average, goes a wavefront a row (amg_wide_rows_kernel)
static_assert(kRowThreads % 64 == 0, "whole wavefronts");

int amg_knob(const char *name, int dflt, int lo, int hi) {
  const char *s = getenv(name);
  if (!s || !*s) return dflt;
  char *end = nullptr;
  const long long v = strtoll(s, &end, 10);
  if (end == s) return dflt;
  return (int)(v < lo ? lo : v > hi ? hi : v);
}

// ---- aggregation --------------------------------------------------------------------------------------------------------
__device__ inline bool precedes(int u, int v, uint64_t base) {  // u != v
  const uint64_t hu = color_priority((uint64_t)u, base), hv = color_priority((uint64_t)v, base);
  return hu > hv || (hu == hv && u < v);
}

// the one of two candidates (-1: none) that precedes the other
__device__ inline int first_of(int a, int b, uint64_t base) {
  if (a < 0 || a == b) return b;
  if (b < 0) return a;
  return precedes(a, b, base) ? a : b;
}

// f(u) for v and every neighbour u of v (a neighbour stored on both sides, or the diagonal, comes twice)
template <typename F>
__device__ inline void closed_neighbourhood(const ColorGraph &g, int v, F &&f) {
  f(v);
  const int e = g.ptr[v + 1];
  for (int q = g.ptr[v]; q < e; ++q) f(g.col[q]);
  const int64_t te = g.tptr[v + 1];
  for (int64_t q = g.tptr[v]; q < te; ++q) f(g.tcol[q]);
}

__global__ __launch_bounds__(kRowThreads) void agg_init_kernel(int n, int *__restrict__ cand, int *__restrict__ state) {
  int64_t v = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; v < n; v += stride) {
    cand[v] = (int)v;  // undecided: the vertex is its own candidate
    state[v] = 0;
  }
}

// launches 1 and 2 of a round: out[v] = the first of in[u], u in N[v]
__global__ __launch_bounds__(kRowThreads) void agg_first_kernel(ColorGraph g, int n, uint64_t base,
                                                                const int *__restrict__ in, int *__restrict__ out) {
  int64_t v = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; v < n; v += stride) {
    int best = -1;
    closed_neighbourhood(g, (int)v, [&](int u) { best = first_of(best, in[u], base); });
    out[v] = best;
  }
}

// launch 3: a root of this round is in N[v]
__global__ __launch_bounds__(kRowThreads) void agg_near_kernel(ColorGraph g, int n, const int *__restrict__ cand,
                                                               const int *__restrict__ best2, int *__restrict__ near) {
  int64_t v = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; v < n; v += stride) {
    int any = 0;
    closed_neighbourhood(g, (int)v, [&](int u) { any |= (cand[u] == u && best2[u] == u); });
    near[v] = any;
  }
}

// launch 4: roots, the vertices that are out, and the number of those that stay undecided
__global__ __launch_bounds__(kRowThreads) void agg_decide_kernel(ColorGraph g, int n, const int *__restrict__ best2,
                                                                 const int *__restrict__ near, int *cand,
                                                                 int *__restrict__ state, int *__restrict__ undecided) {
  __shared__ int staying;
  if (threadIdx.x == 0) staying = 0;
  __syncthreads();
  int64_t v = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  int mine = 0;
  for (; v < n; v += stride) {
    if (cand[v] != (int)v) continue;  // decided in an earlier round
    if (best2[v] == (int)v) {
      state[v] = 1;
      cand[v] = -1;
      continue;
    }
    int out = 0;
    closed_neighbourhood(g, (int)v, [&](int u) { out |= near[u]; });
    if (out) {
      state[v] = 2;
      cand[v] = -1;
    } else {
      ++mine;
    }
  }
  if (mine) atomicAdd(&staying, mine);
  __syncthreads();
  if (threadIdx.x == 0 && staying) atomicAdd(undecided, staying);
}

__global__ __launch_bounds__(kRowThreads) void agg_root_flags_kernel(int n, const int *__restrict__ state,
                                                                     int *__restrict__ flags) {
  int64_t v = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; v < n; v += stride) flags[v] = state[v] == 1;
}

// phase 1: a root takes its number, a neighbour of a root that root's (two roots are never within distance 2)
__global__ __launch_bounds__(kRowThreads) void agg_phase1_kernel(ColorGraph g, int n, const int *__restrict__ state,
                                                                 const int64_t *__restrict__ number,
                                                                 int *__restrict__ first, int *__restrict__ roots) {
  int64_t v = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; v < n; v += stride) {
    int a = -1;
    if (state[v] == 1) {
      a = (int)number[v];
      if (roots) roots[a] = (int)v;
    } else {
      closed_neighbourhood(g, (int)v, [&](int u) {
        if (state[u] == 1) a = (int)number[u];
      });
    }
    first[v] = a;
  }
}

// phase 2: the others take the aggregate of the phase-1 neighbour that precedes the rest; the sizes
__global__ __launch_bounds__(kRowThreads) void agg_phase2_kernel(ColorGraph g, int n, uint64_t base,
                                                                 const int *__restrict__ first, int *__restrict__ agg,
                                                                 int *__restrict__ sizes, int *__restrict__ late) {
  int64_t v = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; v < n; v += stride) {
    int a = first[v];
    if (a < 0) {
      int best = -1;
      closed_neighbourhood(g, (int)v, [&](int u) {
        if (first[u] >= 0) best = first_of(best, u, base);
      });
      if (best >= 0) a = first[best];  // one exists: the roots are a MAXIMAL set
      atomicAdd(late, 1);
    }
    agg[v] = a;
    if (a >= 0) atomicAdd(&sizes[a], 1);
  }
}

__global__ __launch_bounds__(kRowThreads) void agg_extent_kernel(const int *__restrict__ sizes, int count,
                                                                 int *__restrict__ extent) {
  int64_t k = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  int most = 0, least = INT_MAX;
  for (; k < count; k += stride) {
    most = max(most, sizes[k]);
    least = min(least, sizes[k]);
  }
  if (most > 0) {
    atomicMax(&extent[0], most);
    atomicMin(&extent[1], least);
  }
}

}  // namespace

int aggregate_handle(const Matrix *A, uint64_t seed, int *d_agg, int *d_roots, int64_t info[8]) {
  hipStream_t s = nullptr;
  const int n = (int)A->nrows_local;
  for (int k = 0; k < 8; ++k) info[k] = 0;
  info[0] = n;
  if (n == 0) return SPL_OK;
  const int check_every = amg_knob("SPL_AMG_CHECK_EVERY", kAmgCheckEveryDefault, 1, kAmgCheckEveryMax);
  const int64_t grid_cap = amg_knob("SPL_AMG_GRID", kAmgGridDefault, 1, 1 << 16);
  const unsigned grid = grid_flat(n, grid_cap);
  const uint64_t base = kColorGolden * (seed + 1);
  int64_t launches = 0, shared_launches = 0;

  ColorGraphBuffers sides;
  const ColorGraph graph = build_color_graph(A, grid_cap, sides, &shared_launches, s);
  DBuf<int> scalars(4);  // [0] largest degree, [1] largest aggregate, [2] smallest, [3] vertices of phase 2
  const int start[4] = {0, 0, INT_MAX, 0};
  SPL_HIP(hipMemcpyAsync(scalars.get(), start, sizeof(start), hipMemcpyHostToDevice, s));
  color_graph_max_degree(graph, n, group_for((double)A->nnz / (double)n), grid_cap, scalars.get(), s);
  SPL_HIP(hipGetLastError());

  // the rounds
  DBuf<int> cand((size_t)n), state((size_t)n), best1((size_t)n), best2((size_t)n), near((size_t)n);
  DBuf<int> count((size_t)check_every);
  std::vector<int> seen((size_t)check_every, 0);
  hipLaunchKernelGGL(agg_init_kernel, dim3(grid), dim3(kRowThreads), 0, s, n, cand.get(), state.get());
  ++launches;
  int64_t rounds = 0;
  for (bool open = true; open;) {
    SPL_HIP(hipMemsetAsync(count.get(), 0, (size_t)check_every * sizeof(int), s));
    for (int k = 0; k < check_every; ++k) {
      hipLaunchKernelGGL(agg_first_kernel, dim3(grid), dim3(kRowThreads), 0, s, graph, n, base, cand.get(), best1.get());
      hipLaunchKernelGGL(agg_first_kernel, dim3(grid), dim3(kRowThreads), 0, s, graph, n, base, best1.get(), best2.get());
      hipLaunchKernelGGL(agg_near_kernel, dim3(grid), dim3(kRowThreads), 0, s, graph, n, cand.get(), best2.get(), near.get());
      hipLaunchKernelGGL(agg_decide_kernel, dim3(grid), dim3(kRowThreads), 0, s, graph, n, best2.get(), near.get(),
                         cand.get(), state.get(), count.get() + k);
      launches += 4;
    }
    SPL_HIP(hipGetLastError());
    SPL_HIP(hipMemcpyAsync(seen.data(), count.get(), (size_t)check_every * sizeof(int), hipMemcpyDeviceToHost, s));
    SPL_HIP(hipStreamSynchronize(s));
    int k = 0;
    while (k < check_every && seen[(size_t)k] > 0) ++k;
    if (k < check_every) {  // round k of the batch left nobody undecided; the ones behind it did nothing
      rounds += k + 1;
      open = false;
    } else {
      rounds += check_every;
    }
  }

  // the roots in ascending index, the two phases
  DBuf<int64_t> number((size_t)n + 1);
  hipLaunchKernelGGL(agg_root_flags_kernel, dim3(grid), dim3(kRowThreads), 0, s, n, state.get(), best1.get());
  exclusive_scan_i32_to_i64(best1.get(), number.get(), n, s);
  int64_t naggr = 0;
  SPL_HIP(hipMemcpyAsync(&naggr, number.get() + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  DBuf<int> sizes((size_t)naggr);
  SPL_HIP(hipMemsetAsync(sizes.get(), 0, (size_t)naggr * sizeof(int), s));
  hipLaunchKernelGGL(agg_phase1_kernel, dim3(grid), dim3(kRowThreads), 0, s, graph, n, state.get(), number.get(),
                     best2.get(), d_roots);
  hipLaunchKernelGGL(agg_phase2_kernel, dim3(grid), dim3(kRowThreads), 0, s, graph, n, base, best2.get(), d_agg,
                     sizes.get(), scalars.get() + 3);
  hipLaunchKernelGGL(agg_extent_kernel, dim3(grid_flat(naggr, grid_cap)), dim3(kRowThreads), 0, s, sizes.get(),
                     (int)naggr, scalars.get() + 1);
  launches += 4;
  SPL_HIP(hipGetLastError());
  int got[4] = {0, 0, 0, 0};
  SPL_HIP(hipMemcpyAsync(got, scalars.get(), sizeof(got), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));  // the buffers go on return
  info[1] = naggr;
  info[2] = rounds;
  info[3] = got[1];
  info[4] = got[2];
  info[5] = got[0];
  info[6] = launches;
  info[7] = got[3];
  return SPL_OK;
}

// ---- the hierarchy ------------------------------------------------------------------------------------------------------
namespace {

__device__ inline Val<1> vadd(Val<1> a, Val<1> b) { return Val<1>{a.re + b.re}; }
__device__ inline Val<2> vadd(Val<2> a, Val<2> b) { return Val<2>{a.re + b.re, a.im + b.im}; }
__device__ inline Val<1> one_of(Val<1>) { return Val<1>{1.0}; }
__device__ inline Val<2> one_of(Val<2>) { return Val<2>{1.0, 0.0}; }
__device__ inline Val<1> real_of(Val<1>, double v) { return Val<1>{v}; }
__device__ inline Val<2> real_of(Val<2>, double v) { return Val<2>{v, 0.0}; }
__device__ inline bool zero_val(Val<1> a) { return a.re == 0.0; }
__device__ inline bool zero_val(Val<2> a) { return a.re == 0.0 && a.im == 0.0; }

// dinv = 1 / d (the IEEE quotient, Data.Complex's on packed pairs); *zero_seen |= 1 when some d_i is zero
template <int VW>
__global__ __launch_bounds__(kRowThreads) void amg_reciprocal_kernel(int64_t n, const double *__restrict__ d,
                                                                     double *__restrict__ dinv, int *zero_seen) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  int seen = 0;
  for (; i < n; i += stride) {
    const Val<VW> di = load_val<VW>(d, i);
    seen |= zero_val(di);
    store_val(dinv, i, quot(one_of(Val<VW>()), di));
  }
  if (seen) atomicOr(zero_seen, 1);
}

// w = omega dinv: (omega :+ 0) times dinv by Data.Complex's product on packed pairs
template <int VW>
__global__ __launch_bounds__(kRowThreads) void amg_weights_kernel(int64_t n, double omega, const double *__restrict__ dinv,
                                                                  double *__restrict__ w) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; i < n; i += stride) store_val(w, i, mul(real_of(Val<VW>(), omega), load_val<VW>(dinv, i)));
}

// the arrays of T beside the aggregates: the pointers 0 ... n and n ones
template <int VW>
__global__ __launch_bounds__(kRowThreads) void amg_tentative_kernel(int64_t n, int *__restrict__ ptr,
                                                                    double *__restrict__ ones) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; i <= n; i += stride) {
    ptr[i] = (int)i;
    if (i < n) store_val(ones, i, one_of(Val<VW>()));
  }
}

// ---- the cycle's vector steps on the large levels: one pass each ---------------------------------------------------------
// x = w (.) b
template <int VW>
__global__ __launch_bounds__(kRowThreads) void amg_scale_kernel(int64_t n, const double *__restrict__ w,
                                                                const double *__restrict__ b, double *__restrict__ x) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; i < n; i += stride) store_val(x, i, mul(load_val<VW>(w, i), load_val<VW>(b, i)));
}

// x += w (.) (b - t)
template <int VW>
__global__ __launch_bounds__(kRowThreads) void amg_sweep_kernel(int64_t n, const double *__restrict__ w,
                                                                const double *__restrict__ b, const double *__restrict__ t,
                                                                double *__restrict__ x) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; i < n; i += stride) {
    const Val<VW> diff = sub(load_val<VW>(b, i), load_val<VW>(t, i));
    store_val(x, i, vadd(load_val<VW>(x, i), mul(load_val<VW>(w, i), diff)));
  }
}

// r = b - t
template <int VW>
__global__ __launch_bounds__(kRowThreads) void amg_residual_kernel(int64_t n, const double *__restrict__ b,
                                                                   const double *__restrict__ t, double *__restrict__ r) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; i < n; i += stride) store_val(r, i, sub(load_val<VW>(b, i), load_val<VW>(t, i)));
}

// y = R x for an R of few, long rows (the restriction above the small levels: 365 rows of 400 entries took the
// row-per-lane SpMV 565 us, one dependent gather after the other).  A wavefront takes a row: the 64 lanes form 64
// products at once, each rounded on its own, and every lane then adds them in ascending column order from +0.0 —
// the sum of the serial walk, bit for bit, whatever the row's length: spl_matrix_spmv_dev's caveat for rows of more
// than 512 entries does not apply to this product.
template <int VW>
__global__ __launch_bounds__(kRowThreads) void amg_wide_rows_kernel(int nrows, const int *__restrict__ ptr,
                                                                    const int *__restrict__ col,
                                                                    const double *__restrict__ val,
                                                                    const double *__restrict__ x, double *__restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (kRowThreads / 64) + (threadIdx.x >> 6);
  if (row >= nrows) return;  // the whole wavefront leaves
  const int s = ptr[row], e = ptr[row + 1];
  Val<VW> acc = Val<VW>();
  for (int base = s; base < e; base += 64) {
    const int q = base + lane;
    Val<VW> p = Val<VW>();
    if (q < e) p = mul(load_val<VW>(val, q), load_val<VW>(x, col[q]));
    const int held = min(64, e - base);
    for (int k = 0; k < held; ++k) acc = vadd(acc, from_lane<64>(p, k));
  }
  if (lane == 0) store_val(y, row, acc);
}

// ---- the tail: the sub-cycle of the small levels in one workgroup ---------------------------------------------------------
struct TailLevel {
  int n, nc;  // rows, and rows of the next level (0 on the coarsest)
  const int *Ap, *Ac, *Pp, *Pc, *Rp, *Rc;
  const double *Av, *Pv, *Rv, *w;
  double *x, *b, *t, *r;  // the level's work vectors; the first tail level's b and x are the launch's arguments
};

// acc + sum of a_ij x_j over row i in ascending column order, product and sum rounded apart
template <int VW>
__device__ inline Val<VW> tail_row(const int *ptr, const int *col, const double *val, int i, const double *x, Val<VW> acc) {
  const int e = ptr[i + 1];
  for (int q = ptr[i]; q < e; ++q) acc = vadd(acc, mul(load_val<VW>(val, q), load_val<VW>(x, col[q])));
  return acc;
}

// No __restrict__ on the vectors: every step reads what the step before it wrote, behind a workgroup barrier
template <int VW>
__global__ __launch_bounds__(kTailThreads) void amg_tail_kernel(const TailLevel *levels, int count, int nu, int coarse,
                                                                const double *b0, double *x0) {
  const int lane = threadIdx.x, lanes = blockDim.x;
  auto sweep = [&](const TailLevel &L, const double *b, double *x) {
    for (int i = lane; i < L.n; i += lanes) store_val(L.t, i, tail_row<VW>(L.Ap, L.Ac, L.Av, i, x, Val<VW>()));
    __syncthreads();
    for (int i = lane; i < L.n; i += lanes) {
      const Val<VW> diff = sub(load_val<VW>(b, i), load_val<VW>(L.t, i));
      store_val(x, i, vadd(load_val<VW>(x, i), mul(load_val<VW>(L.w, i), diff)));
    }
    __syncthreads();
  };
  // down
  for (int l = 0; l < count; ++l) {
    const TailLevel L = levels[l];
    const double *b = l == 0 ? b0 : L.b;
    double *x = l == 0 ? x0 : L.x;
    for (int i = lane; i < L.n; i += lanes) store_val(x, i, mul(load_val<VW>(L.w, i), load_val<VW>(b, i)));
    __syncthreads();
    const bool coarsest = l == count - 1;
    const int more = coarsest ? coarse - 1 : nu - 1;
    for (int k = 0; k < more; ++k) sweep(L, b, x);
    if (coarsest) break;
    for (int i = lane; i < L.n; i += lanes) {
      const Val<VW> ti = tail_row<VW>(L.Ap, L.Ac, L.Av, i, x, Val<VW>());
      store_val(L.r, i, sub(load_val<VW>(b, i), ti));
    }
    __syncthreads();
    double *next_b = levels[l + 1].b;
    for (int i = lane; i < L.nc; i += lanes) store_val(next_b, i, tail_row<VW>(L.Rp, L.Rc, L.Rv, i, L.r, Val<VW>()));
    __syncthreads();
  }
  // up
  for (int l = count - 2; l >= 0; --l) {
    const TailLevel L = levels[l];
    const double *b = l == 0 ? b0 : L.b;
    double *x = l == 0 ? x0 : L.x;
    const double *e = levels[l + 1].x;
    for (int i = lane; i < L.n; i += lanes) store_val(x, i, tail_row<VW>(L.Pp, L.Pc, L.Pv, i, e, load_val<VW>(x, i)));
    __syncthreads();
    for (int k = 0; k < nu; ++k) sweep(L, b, x);
  }
}

struct AmgLevel {
  Matrix *A = nullptr, *P = nullptr, *R = nullptr;  // P and R nullptr on the coarsest level
  bool owns_A = false;                              // level 0 borrows the caller's handle
  int64_t n = 0;
  DBuf<double> w;                                   // n entries
  DBuf<double> work;                                // x, b, t, r
  double *vec(int i, int vw) const { return work.get() + (size_t)i * (size_t)n * (size_t)vw; }
};

size_t matrix_bytes(const Matrix *m) {
  return (size_t)m->nnz * (sizeof(int) + (size_t)m->vw * sizeof(double)) +
         ((size_t)m->nrows_local + 1) * (sizeof(int64_t) + sizeof(int));
}

void free_handle(Matrix *&m) {
  void *h = m;
  if (h) spl_matrix_free(&h);
  m = nullptr;
}

struct Status {
  int st;
};
void must(int st) {
  if (st < 0) throw Status{st};
}

}  // namespace

struct Amg : ObjectHead {
  Amg() : ObjectHead(kAmgMagic) {}
  uint64_t seed = 0;
  int nu = 1, coarse_sweeps = 4, max_levels = 16, plain = 0;
  int64_t coarse_size = 256;
  std::vector<AmgLevel> levels;
  int tail_first = -1;
  int tail_threads = 64;             // a lane a row of the largest tail level, in whole wavefronts
  DBuf<TailLevel> tail;
  int64_t flags = 0;
  size_t bytes = 0;
  std::mutex lock;                   // one application is enqueued at a time
  hipEvent_t applied = nullptr;      // behind the last kernel of the last application
  hipStream_t applied_on = nullptr;
  bool in_use = false;
  ~Amg() {
    for (AmgLevel &L : levels) {
      if (L.owns_A) free_handle(L.A);
      free_handle(L.P);
      free_handle(L.R);
    }
    if (applied) (void)hipEventDestroy(applied);
  }
};

namespace {

// w of the level, and whether a zero stands on its diagonal
template <int VW>
void level_weights(Amg *M, AmgLevel &L, int *d_zero_seen) {
  hipStream_t s = nullptr;
  const int64_t n = L.n;
  L.w.alloc((size_t)n * VW);
  if (n == 0) return;
  DBuf<double> d((size_t)n * VW), dinv((size_t)n * VW);
  must(spl_matrix_take_diag_dev(L.A, d.get(), s));
  hipLaunchKernelGGL((amg_reciprocal_kernel<VW>), dim3(grid_flat(n, kVectorGrid)), dim3(kRowThreads), 0, s, n, d.get(),
                     dinv.get(), d_zero_seen);
  SPL_HIP(hipGetLastError());
  void *scaled = nullptr;
  must(spl_matrix_scale_rows_cols(L.A, dinv.get(), nullptr, &scaled));
  double nrm = 0.0;
  const int st = spl_matrix_norm(scaled, SPL_NORM_inf, &nrm);
  spl_matrix_free(&scaled);
  must(st);
  const double three = 3.0 * nrm;
  const double omega = 4.0 / three;
  hipLaunchKernelGGL((amg_weights_kernel<VW>), dim3(grid_flat(n, kVectorGrid)), dim3(kRowThreads), 0, s, n, omega,
                     dinv.get(), L.w.get());
  SPL_HIP(hipGetLastError());
  SPL_HIP(hipStreamSynchronize(s));  // d and dinv go on return
}

// P, R and the next level's A from the level's aggregates
template <int VW>
void coarsen(Amg *M, AmgLevel &L, const int *d_agg, int64_t naggr, Matrix **next) {
  hipStream_t s = nullptr;
  const int64_t n = L.n;
  DBuf<int> ptr((size_t)n + 1);
  DBuf<double> ones((size_t)n * VW);
  hipLaunchKernelGGL((amg_tentative_kernel<VW>), dim3(grid_flat(n + 1, kVectorGrid)), dim3(kRowThreads), 0, s, n, ptr.get(),
                     ones.get());
  SPL_HIP(hipGetLastError());
  SPL_HIP(hipStreamSynchronize(s));
  void *T = nullptr, *WA = nullptr, *WAT = nullptr, *P = nullptr, *R = nullptr, *AP = nullptr, *RAP = nullptr;
  int st = spl_matrix_create_csr_dev(n, naggr, 4, ptr.get(), d_agg, ones.get(), VW, &T);
  if (st >= 0 && M->plain) {
    P = T;
    T = nullptr;
  } else if (st >= 0) {
    const double one[2] = {1.0, 0.0}, minus[2] = {-1.0, 0.0};
    st = spl_matrix_scale_rows_cols(L.A, L.w.get(), nullptr, &WA);
    if (st >= 0) st = spl_matrix_spgemm(WA, T, &WAT, nullptr);
    if (st >= 0) st = spl_matrix_lin(T, one, WAT, minus, &P);
  }
  if (st >= 0) st = VW == 2 ? spl_matrix_ctrans(P, &R) : spl_matrix_transpose(P, &R);
  if (st >= 0) st = spl_matrix_spgemm(L.A, P, &AP, nullptr);
  if (st >= 0) st = spl_matrix_spgemm(R, AP, &RAP, nullptr);
  spl_matrix_free(&T);
  spl_matrix_free(&WA);
  spl_matrix_free(&WAT);
  spl_matrix_free(&AP);
  L.P = static_cast<Matrix *>(P);
  L.R = static_cast<Matrix *>(R);
  *next = static_cast<Matrix *>(RAP);
  must(st);
}

template <int VW>
void build_hierarchy(Amg *M, Matrix *A) {
  DBuf<int> zero_seen(1);
  SPL_HIP(hipMemsetAsync(zero_seen.get(), 0, sizeof(int), nullptr));
  Matrix *cur = A;
  for (int l = 0;; ++l) {
    M->levels.emplace_back();
    AmgLevel &L = M->levels.back();
    L.A = cur;
    L.owns_A = l > 0;
    L.n = cur->nrows_local;
    level_weights<VW>(M, L, zero_seen.get());
    L.work.alloc(4 * (size_t)L.n * VW);
    if (L.n <= M->coarse_size || l + 1 == M->max_levels) break;
    if (cur->nnz >= (int64_t)0x7fffffff || !cur->rowptr.get()) throw Status{SPL_ERROR_index_overflow};
    DBuf<int> agg((size_t)L.n);
    int64_t info[8];
    must(aggregate_handle(cur, M->seed, agg.get(), nullptr, info));
    if (info[1] == L.n) break;  // no vertex has a neighbour: nothing to merge
    Matrix *next = nullptr;
    try {
      coarsen<VW>(M, L, agg.get(), info[1], &next);
    } catch (...) {
      free_handle(next);
      throw;
    }
    cur = next;
  }
  int seen = 0;
  SPL_HIP(hipMemcpy(&seen, zero_seen.get(), sizeof(int), hipMemcpyDeviceToHost));
  M->flags = (seen ? 1 : 0) | (VW == 2 ? 2 : 0);
}

bool fits_tail(const AmgLevel &L, int64_t tail_rows) {
  if (L.n > tail_rows) return false;
  for (const Matrix *m : {(const Matrix *)L.A, (const Matrix *)L.P, (const Matrix *)L.R})
    if (m && (m->max_row_len > kTailRowLen || !m->rowptr.get())) return false;
  return true;
}

void plan_tail(Amg *M) {
  const int64_t tail_rows = amg_knob("SPL_AMG_TAIL_ROWS", kTailRowsMax, 0, kTailRowsMax);
  const int count = (int)M->levels.size();
  int first = count;
  while (first > 0 && tail_rows > 0 && fits_tail(M->levels[(size_t)first - 1], tail_rows)) --first;
  if (first == count) return;
  std::vector<TailLevel> table;
  for (int l = first; l < count; ++l) {
    const AmgLevel &L = M->levels[(size_t)l];
    TailLevel t;
    memset(&t, 0, sizeof(t));
    t.n = (int)L.n;
    t.Ap = L.A->rowptr.get(), t.Ac = L.A->colidx.get(), t.Av = L.A->val.get();
    if (L.P) {
      t.nc = (int)L.R->nrows_local;
      t.Pp = L.P->rowptr.get(), t.Pc = L.P->colidx.get(), t.Pv = L.P->val.get();
      t.Rp = L.R->rowptr.get(), t.Rc = L.R->colidx.get(), t.Rv = L.R->val.get();
    }
    t.w = L.w.get();
    t.x = L.vec(0, M->vw), t.b = L.vec(1, M->vw), t.t = L.vec(2, M->vw), t.r = L.vec(3, M->vw);
    table.push_back(t);
    const int threads = (int)((L.n + 63) / 64 * 64);
    M->tail_threads = std::min(kTailThreads, std::max(M->tail_threads, threads));
  }
  M->tail.alloc(table.size());
  SPL_HIP(hipMemcpy(M->tail.get(), table.data(), table.size() * sizeof(TailLevel), hipMemcpyHostToDevice));
  M->tail_first = first;
}

}  // namespace

int amg_create(Matrix *A, const int64_t opt[8], Amg **out) {
  std::unique_ptr<Amg> M(new Amg);
  M->device = A->device;
  M->vw = A->vw;
  M->n = A->nrows_local;
  M->seed = (uint64_t)opt[0];
  M->nu = (int)opt[1];
  M->coarse_size = opt[2];
  M->max_levels = (int)opt[3];
  M->coarse_sweeps = (int)opt[4];
  M->plain = (int)(opt[5] & 1);
  M->levels.reserve((size_t)M->max_levels);  // a level is referred to while the next one is made
  try {
    if (M->vw == 1) build_hierarchy<1>(M.get(), A);
    else build_hierarchy<2>(M.get(), A);
  } catch (const Status &e) {
    return e.st;
  }
  plan_tail(M.get());
  SPL_HIP(hipEventCreateWithFlags(&M->applied, hipEventDisableTiming));
  size_t bytes = M->tail.n * sizeof(TailLevel);
  for (const AmgLevel &L : M->levels) {
    bytes += (L.w.n + L.work.n) * sizeof(double);
    if (L.owns_A) bytes += matrix_bytes(L.A);
    if (L.P) bytes += matrix_bytes(L.P) + matrix_bytes(L.R);
  }
  M->bytes = bytes;
  *out = M.release();
  return SPL_OK;
}

void amg_info(Amg *M, int64_t info[8]) {
  int64_t total = 0;
  for (const AmgLevel &L : M->levels) total += L.A->nnz;
  info[0] = M->n;
  info[1] = (int64_t)M->levels.size();
  info[2] = total;
  info[3] = M->levels.front().A->nnz;
  info[4] = M->levels.back().n;
  info[5] = M->tail_first;
  info[6] = (int64_t)M->bytes;
  info[7] = M->flags;
}

void amg_level(Amg *M, int level, void **HA, void **HP, void **HR, const double **d_w, int64_t dims[2]) {
  const AmgLevel &L = M->levels[(size_t)level];
  if (HA) *HA = L.A;
  if (HP) *HP = L.P;
  if (HR) *HR = L.R;
  if (d_w) *d_w = L.w.get();
  if (dims) {
    dims[0] = L.n;
    dims[1] = L.R ? L.R->nrows_local : 0;
  }
}

namespace {

template <int VW>
struct CycleRun {
  Amg *M;
  hipStream_t s;
  int64_t launches = 0;

  int sweep(const AmgLevel &L, const double *b, double *x) {
    double *t = L.vec(2, VW);
    const int e = launch_spmv(L.A, x, t, 0, s);
    if (e != SPL_OK) return e;
    hipLaunchKernelGGL((amg_sweep_kernel<VW>), dim3(grid_flat(L.n, kVectorGrid)), dim3(kRowThreads), 0, s, L.n, L.w.get(), b,
                       t, x);
    launches += 2;
    return SPL_OK;
  }

  int cycle(int l, const double *b, double *x) {
    const AmgLevel &L = M->levels[(size_t)l];
    if (l == M->tail_first) {
      hipLaunchKernelGGL((amg_tail_kernel<VW>), dim3(1), dim3(M->tail_threads), 0, s, (const TailLevel *)M->tail.get(),
                         (int)M->levels.size() - l, M->nu, M->coarse_sweeps, b, x);
      ++launches;
      return SPL_OK;
    }
    const unsigned grid = grid_flat(L.n, kVectorGrid);
    int e;
    hipLaunchKernelGGL((amg_scale_kernel<VW>), dim3(grid), dim3(kRowThreads), 0, s, L.n, L.w.get(), b, x);
    ++launches;
    const bool coarsest = l + 1 == (int)M->levels.size();
    const int more = coarsest ? M->coarse_sweeps - 1 : M->nu - 1;
    for (int k = 0; k < more; ++k)
      if ((e = sweep(L, b, x)) != SPL_OK) return e;
    if (coarsest) return SPL_OK;
    double *t = L.vec(2, VW), *r = L.vec(3, VW);
    const AmgLevel &N = M->levels[(size_t)l + 1];
    double *nx = N.vec(0, VW), *nb = N.vec(1, VW);
    if ((e = launch_spmv(L.A, x, t, 0, s)) != SPL_OK) return e;
    hipLaunchKernelGGL((amg_residual_kernel<VW>), dim3(grid), dim3(kRowThreads), 0, s, L.n, b, t, r);
    const Matrix *R = L.R;
    if (R->nrows_local <= kWideRowsMax && R->nnz >= kWideRowsMean * R->nrows_local) {
      const int rows = (int)R->nrows_local;
      hipLaunchKernelGGL((amg_wide_rows_kernel<VW>), dim3((unsigned)((rows + 3) / 4)), dim3(kRowThreads), 0, s, rows,
                         R->rowptr.get(), R->colidx.get(), R->val.get(), r, nb);
    } else if ((e = launch_spmv(R, r, nb, 0, s)) != SPL_OK) {
      return e;
    }
    launches += 3;
    if ((e = cycle(l + 1, nb, nx)) != SPL_OK) return e;
    if ((e = launch_spmv(L.P, nx, x, 1, s)) != SPL_OK) return e;
    ++launches;
    for (int k = 0; k < M->nu; ++k)
      if ((e = sweep(L, b, x)) != SPL_OK) return e;
    return SPL_OK;
  }
};

}  // namespace

int amg_apply(Amg *M, const double *d_b, double *d_x, hipStream_t s, int64_t *launches) {
  if (launches) *launches = 0;
  if (M->n == 0) return SPL_OK;
  std::lock_guard<std::mutex> hold(M->lock);
  // the work vectors are the object's: an application on another stream starts behind the one before it
  if (M->in_use && M->applied_on != s) SPL_HIP(hipStreamWaitEvent(s, M->applied, 0));
  int e;
  int64_t count = 0;
  if (M->vw == 1) {
    CycleRun<1> run{M, s};
    e = run.cycle(0, d_b, d_x);
    count = run.launches;
  } else {
    CycleRun<2> run{M, s};
    e = run.cycle(0, d_b, d_x);
    count = run.launches;
  }
  if (launches) *launches = count;
  const hipError_t le = hipGetLastError();
  if (e == SPL_OK && le != hipSuccess) {
    set_last_error("amg cycle launch", le);
    e = SPL_ERROR_device;
  }
  if (hipEventRecord(M->applied, s) != hipSuccess) (void)hipStreamSynchronize(s);
  M->applied_on = s;
  M->in_use = true;
  if (e != SPL_OK) (void)hipStreamSynchronize(s);
  return e;
}

void amg_delete(Amg *M) {
  if (M->applied) (void)hipEventSynchronize(M->applied);
  delete_object(M);
}

}  // namespace spl

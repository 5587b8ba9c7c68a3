// coloring.hip — multicolour ordering on device handles: a distance-1 colouring of the adjacency graph of a whole square
// handle, the permutation that numbers the unknowns colour by colour, and the kernel that moves vectors along it.  A row
// of the lower triangle of P A P^T then depends on rows of earlier colours only, so the triangular solves and ILU(0)
// (trisolve.hip, ilu0.hip) find at most as many levels as there are colours; their kernels are not touched.
//
// Contract (include/sparse_linear_hip.h): {i, j}, i != j, is an edge when a_ij or a_ji is stored (values are never read).
// h(v) is the splitmix64 finaliser of v + 0x9E3779B97F4A7C15 (seed + 1); u precedes v when h(u) > h(v), or they are equal
// and u < v.  colour(v) = the smallest c >= 0 that no neighbour preceding v has: the serial first-fit colouring in
// priority order, which is the fixed point of Jones-Plassmann rounds.  round(v) = 1 + max round over the preceding
// neighbours.  Both are functions of the pattern and the seed alone, and that is what the kernels below produce, whatever
// the grid, the worklist's order and the host's looks at the count are.
//
// One launch is one round.  A vertex of the worklist whose preceding neighbours all carried a colour when the launch
// began takes its colour; the others go to the next worklist.  Round and colour live in ONE aligned 8-byte word per
// vertex (round << 32 | colour, 0: none yet), written by one store: a neighbour whose word carries the current round
// was coloured in this launch and counts as uncoloured, so a vertex never profits from a colour of its own round
// whether it sees the fresh word or the old one.  No kernel waits for another workgroup; the integer atomics hand out
// worklist slots, and nothing in the result depends on their order.
//
// The smallest free colour goes through a 64-bit mask per window of 64 colours, in registers: when windows 0 ... w-1
// are full the row is walked again for window w, so any degree is served without scratch memory.  A vertex is worked by
// a group of G lanes (row_groups.hpp) over row v of A followed by row v of A^T's pattern; mask and readiness are
// combined by shuffles.  A^T's pattern is built here without values and without order inside a row: a set is all the
// colouring reads.
#include <algorithm>

#include "row_groups.hpp"

namespace spl {
namespace {

constexpr uint64_t kGolden = kColorGolden;
constexpr int kCheckEveryDefault = 8, kCheckEveryMax = 4096;
constexpr int kHistBins = 256;  // colours counted in LDS; higher ones go to memory one by one
constexpr int kPending = 1024;  // waiting vertices a workgroup collects in LDS before they go to the next worklist
constexpr int kGridDefault = 2048;  // workgroups of a launch at most: eight per CU

__host__ __device__ inline uint64_t priority(uint64_t v, uint64_t base) { return color_priority(v, base); }

template <int G>
__device__ inline unsigned long long group_or(unsigned long long v) {
#pragma unroll
  for (int w = 1; w < G; w <<= 1) v |= __shfl_xor(v, w, G);
  return v;
}

__global__ __launch_bounds__(kRowThreads) void color_count_columns_kernel(const int *__restrict__ col, int64_t nnz,
                                                                          int *__restrict__ count) {
  int64_t q = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; q < nnz; q += stride) atomicAdd(&count[col[q]], 1);
}

// entry (i, j) of A becomes entry i of row j of the transposed pattern, at the slot an integer atomic hands out
template <int G>
__global__ __launch_bounds__(kRowThreads) void color_fill_transpose_kernel(const int *__restrict__ ptr,
                                                                           const int *__restrict__ col, int n,
                                                                           const int64_t *__restrict__ tptr,
                                                                           int *__restrict__ cursor, int *__restrict__ tcol) {
  constexpr int kGroups = kRowThreads / G;
  const int lane = threadIdx.x % G;
  int64_t i = (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  for (; i < n; i += stride) {
    const int e = ptr[i + 1];
    for (int q = ptr[i] + lane; q < e; q += G) {
      const int j = col[q];
      tcol[tptr[j] + atomicAdd(&cursor[j], 1)] = (int)i;
    }
  }
}

// the largest number of distinct neighbours: the off-diagonal entries of row v, and those of column v that row v does
// not store (the rows of A ascend)
template <int G>
__global__ __launch_bounds__(kRowThreads) void color_degree_kernel(ColorGraph g, int n, int *__restrict__ max_degree) {
  constexpr int kGroups = kRowThreads / G;
  const int lane = threadIdx.x % G;
  int64_t v = (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  int most = 0;
  for (; v < n; v += stride) {
    const int s = g.ptr[v], e = g.ptr[v + 1];
    int degree = 0;
    for (int q = s + lane; q < e; q += G) degree += g.col[q] != (int)v;
    const int64_t te = g.tptr[v + 1];
    for (int64_t q = g.tptr[v] + lane; q < te; q += G) {
      const int u = g.tcol[q];
      if (u == (int)v) continue;
      const int r = s + count_less(g.col, s, e, u);
      degree += !(r < e && g.col[r] == u);
    }
    degree = group_sum<G>(degree);
    most = max(most, degree);
  }
  if (lane == 0 && most > 0) atomicMax(max_degree, most);
}

// One round.  list == nullptr: the worklist is 0 ... *count_in - 1
template <int G>
__global__ __launch_bounds__(kRowThreads) void color_round_kernel(ColorGraph g, uint64_t base, unsigned round,
                                                                  const int *__restrict__ list,
                                                                  const int *__restrict__ count_in,
                                                                  unsigned long long *state, int *__restrict__ colors,
                                                                  int *__restrict__ next, int *__restrict__ count_out) {
  constexpr int kGroups = kRowThreads / G;
  // The vertices that wait are collected in LDS and go to the next worklist kPending at a time: one atomic on the
  // list's length per flush, not one per vertex (6e6 of them on ONE address took 60 ms at 8.0e6 vertices)
  __shared__ int pending[kPending];
  __shared__ int npending, flush_base;
  if (threadIdx.x == 0) npending = 0;
  __syncthreads();
  auto flush = [&]() {  // every thread of the workgroup is here, behind a barrier
    const int held = npending;
    if (held == 0) return;
    if (threadIdx.x == 0) flush_base = atomicAdd(count_out, held);
    __syncthreads();
    for (int t = threadIdx.x; t < held; t += kRowThreads) next[flush_base + t] = pending[t];
    __syncthreads();
    if (threadIdx.x == 0) npending = 0;
    __syncthreads();
  };
  const int lane = threadIdx.x % G;
  const int total = *count_in;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  for (int64_t first = (int64_t)blockIdx.x * kGroups; first < total; first += stride) {  // the same trips for all
    const int64_t p = first + threadIdx.x / G;
    if (p < total) {
      const int v = list ? list[p] : (int)p;
      const uint64_t hv = priority((uint64_t)v, base);
      const int s = g.ptr[v];
      const int own = g.ptr[v + 1] - s;
      const int64_t ts = g.tptr[v];
      const int64_t len = (int64_t)own + (g.tptr[v + 1] - ts);
      int waiting = 0;
      int window = 0;
      unsigned long long mask;
      for (;;) {
        mask = 0;
        for (int64_t t = lane; t < len; t += G) {
          const int u = t < own ? g.col[s + t] : g.tcol[ts + (t - own)];
          if (u == v) continue;
          const uint64_t hu = priority((uint64_t)u, base);
          if (!(hu > hv || (hu == hv && u < v))) continue;  // v precedes u
          const unsigned long long word = state[u];
          const unsigned r = (unsigned)(word >> 32);
          if (r == 0 || r == round) {  // no colour when this launch began
            waiting = 1;
            continue;
          }
          const int c = (int)(unsigned)word;
          if ((c >> 6) == window) mask |= 1ull << (c & 63);
        }
        waiting = group_sum<G>(waiting);
        mask = group_or<G>(mask);
        if (waiting || mask != ~0ull) break;
        ++window;  // colours 64 window ... 64 window + 63 are all taken: once more for the next 64
      }
      if (lane == 0) {
        if (waiting) {
          pending[atomicAdd(&npending, 1)] = v;
        } else {
          const int c = window * 64 + __ffsll((unsigned long long)~mask) - 1;
          state[v] = ((unsigned long long)round << 32) | (unsigned)c;
          colors[v] = c;
        }
      }
    }
    __syncthreads();
    const bool full = npending > kPending - kGroups;  // the next trip adds kGroups at most
    __syncthreads();                                  // everyone has read it before anyone appends again
    if (full) flush();
  }
  flush();
}

// vertices per colour and the largest colour
__global__ __launch_bounds__(kRowThreads) void color_histogram_kernel(const int *__restrict__ colors, int n,
                                                                      int *__restrict__ hist, int *__restrict__ largest) {
  __shared__ int bins[kHistBins];
  __shared__ int top;
  bins[threadIdx.x] = 0;  // (kRowThreads == kHistBins)
  if (threadIdx.x == 0) top = 0;
  __syncthreads();
  int64_t v = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  int mine = 0;
  for (; v < n; v += stride) {
    const int c = colors[v];
    mine = max(mine, c);
    if (c < kHistBins) atomicAdd(&bins[c], 1);
    else atomicAdd(&hist[c], 1);
  }
  if (mine > 0) atomicMax(&top, mine);
  __syncthreads();
  if (bins[threadIdx.x]) atomicAdd(&hist[threadIdx.x], bins[threadIdx.x]);
  if (threadIdx.x == 0 && top > 0) atomicMax(largest, top);
}
static_assert(kRowThreads == kHistBins, "one thread per LDS bin");

// the stable sort's keys: the colour in the low bits, the vertex above them
__global__ __launch_bounds__(kRowThreads) void color_keys_kernel(const int *__restrict__ colors, int n,
                                                                 unsigned long long *__restrict__ keys) {
  int64_t v = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; v < n; v += stride) keys[v] = ((unsigned long long)v << 32) | (unsigned)colors[v];
}

__global__ __launch_bounds__(kRowThreads) void color_perm_kernel(const unsigned long long *__restrict__ keys, int n,
                                                                 int *__restrict__ perm) {
  int64_t k = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; k < n; k += stride) perm[k] = (int)(keys[k] >> 32);
}

// T: unsigned long long (a double's bits) or ulonglong2 (a packed pair's)
template <typename T>
__global__ __launch_bounds__(kRowThreads) void vector_permute_kernel(int64_t n, const int *__restrict__ perm, int inverse,
                                                                     const T *__restrict__ in, T *__restrict__ out) {
  int64_t k = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  if (inverse) {
    for (; k < n; k += stride) out[perm[k]] = in[k];
  } else {
    for (; k < n; k += stride) out[k] = in[perm[k]];
  }
}

int read_knob(const char *name, int dflt, int lo, int hi) {
  const char *s = getenv(name);
  if (!s || !*s) return dflt;
  char *end = nullptr;
  const long long v = strtoll(s, &end, 10);
  if (end == s) return dflt;
  return (int)(v < lo ? lo : v > hi ? hi : v);
}

template <typename F>
void for_group(int group, F &&f) {
  for_group_and_width(group, 1, [&](auto g, auto) { f(g); });
}

}  // namespace

// The transposed pattern of A (n > 0) into buf, and the view of both sides; aggregation (amg.hip) walks the same graph
ColorGraph build_color_graph(const Matrix *A, int64_t grid_cap, ColorGraphBuffers &buf, int64_t *launches, hipStream_t s) {
  const int n = (int)A->nrows_local;
  const int64_t nnz = A->nnz;
  const int G = group_for((double)nnz / (double)n);
  buf.counts.alloc((size_t)n);
  buf.tcol.alloc((size_t)nnz);
  buf.tptr.alloc((size_t)n + 1);
  SPL_HIP(hipMemsetAsync(buf.counts.get(), 0, (size_t)n * sizeof(int), s));
  if (nnz > 0) {
    hipLaunchKernelGGL(color_count_columns_kernel, dim3(grid_flat(nnz, grid_cap)), dim3(kRowThreads), 0, s,
                       A->colidx.get(), nnz, buf.counts.get());
    ++*launches;
  }
  exclusive_scan_i32_to_i64(buf.counts.get(), buf.tptr.get(), n, s);
  SPL_HIP(hipMemsetAsync(buf.counts.get(), 0, (size_t)n * sizeof(int), s));
  if (nnz > 0) {
    for_group(G, [&](auto g) {
      hipLaunchKernelGGL((color_fill_transpose_kernel<decltype(g)::value>), dim3(grid_rows(n, G, grid_cap)),
                         dim3(kRowThreads), 0, s, A->rowptr.get(), A->colidx.get(), n, buf.tptr.get(), buf.counts.get(),
                         buf.tcol.get());
    });
    ++*launches;
  }
  return ColorGraph{A->rowptr.get(), A->colidx.get(), buf.tptr.get(), buf.tcol.get()};
}

// *d_max_degree (zeroed by the caller) receives the largest number of distinct neighbours; enqueues one launch on s
void color_graph_max_degree(const ColorGraph &graph, int n, int G, int64_t grid_cap, int *d_max_degree, hipStream_t s) {
  for_group(G, [&](auto g) {
    hipLaunchKernelGGL((color_degree_kernel<decltype(g)::value>), dim3(grid_rows(n, G, grid_cap)), dim3(kRowThreads), 0, s,
                       graph, n, d_max_degree);
  });
}

// A: whole, square, 32-bit row pointers (the caller checked); d_colors n ints, d_perm n ints or nullptr, offsets
// nullptr or the place for a malloc()'d array of info[1] + 1 entries.  Default stream; synchronises
int color_handle(const Matrix *A, uint64_t seed, int *d_colors, int *d_perm, int64_t **offsets, int64_t info[8]) {
  hipStream_t s = nullptr;
  const int n = (int)A->nrows_local;
  const int64_t nnz = A->nnz;
  for (int k = 0; k < 8; ++k) info[k] = 0;
  info[0] = n;
  if (n == 0) {
    if (offsets) {
      *offsets = static_cast<int64_t *>(malloc(sizeof(int64_t)));
      if (!*offsets) throw std::bad_alloc();
      (*offsets)[0] = 0;
    }
    return SPL_OK;
  }
  const int check_every = read_knob("SPL_COLOR_CHECK_EVERY", kCheckEveryDefault, 1, kCheckEveryMax);
  const int64_t grid_cap = read_knob("SPL_COLOR_GRID", kGridDefault, 1, 1 << 16);
  const int G = group_for((double)nnz / (double)n);
  int64_t launches = 0;
  const uint64_t base = kGolden * (seed + 1);

  // the transposed pattern
  ColorGraphBuffers sides;
  const ColorGraph graph = build_color_graph(A, grid_cap, sides, &launches, s);
  DBuf<int> scalars(2);  // [0] largest degree, [1] largest colour
  SPL_HIP(hipMemsetAsync(scalars.get(), 0, 2 * sizeof(int), s));
  color_graph_max_degree(graph, n, G, grid_cap, scalars.get(), s);
  ++launches;
  SPL_HIP(hipGetLastError());

  // the rounds: count[k] is the length of the worklist round k of a batch reads, count[k + 1] of the one it writes
  DBuf<unsigned long long> state((size_t)n);
  DBuf<int> lists[2] = {DBuf<int>((size_t)n), DBuf<int>((size_t)n)};
  DBuf<int> count((size_t)check_every + 1);
  std::vector<int> seen((size_t)check_every + 1, 0);
  SPL_HIP(hipMemsetAsync(state.get(), 0, (size_t)n * sizeof(unsigned long long), s));
  SPL_HIP(hipMemcpyAsync(count.get(), &n, sizeof(int), hipMemcpyHostToDevice, s));
  const int *in_list = nullptr;
  int out = 0;
  int64_t rounds = 0;
  int remaining = n;
  while (remaining > 0) {
    SPL_HIP(hipMemsetAsync(count.get() + 1, 0, (size_t)check_every * sizeof(int), s));
    const unsigned grid = grid_rows(remaining, G, grid_cap);
    for (int k = 0; k < check_every; ++k) {
      const unsigned round = (unsigned)(rounds + k + 1);
      for_group(G, [&](auto g) {
        hipLaunchKernelGGL((color_round_kernel<decltype(g)::value>), dim3(grid), dim3(kRowThreads), 0, s, graph, base,
                           round, in_list, count.get() + k, state.get(), d_colors, lists[out].get(), count.get() + k + 1);
      });
      ++launches;
      in_list = lists[out].get();
      out ^= 1;
    }
    SPL_HIP(hipGetLastError());
    SPL_HIP(hipMemcpyAsync(seen.data() + 1, count.get() + 1, (size_t)check_every * sizeof(int), hipMemcpyDeviceToHost, s));
    SPL_HIP(hipStreamSynchronize(s));
    int k = 1;
    while (k <= check_every && seen[(size_t)k] > 0) ++k;
    if (k <= check_every) {  // round k of the batch emptied the worklist; the ones behind it did nothing
      rounds += k;
      remaining = 0;
    } else {
      rounds += check_every;
      remaining = seen[(size_t)check_every];
      SPL_HIP(hipMemcpyAsync(count.get(), count.get() + check_every, sizeof(int), hipMemcpyDeviceToDevice, s));
    }
  }

  // the classes
  int top[2] = {0, 0};
  SPL_HIP(hipMemcpyAsync(top, scalars.get(), sizeof(int), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  const int max_degree = top[0];
  DBuf<int> hist((size_t)std::max(max_degree + 1, kHistBins));  // a colour is at most the degree
  SPL_HIP(hipMemsetAsync(hist.get(), 0, (size_t)std::max(max_degree + 1, kHistBins) * sizeof(int), s));
  hipLaunchKernelGGL(color_histogram_kernel, dim3(grid_flat(n, std::min<int64_t>(grid_cap, 1024))), dim3(kRowThreads), 0,
                     s, d_colors, n, hist.get(), scalars.get() + 1);
  ++launches;
  SPL_HIP(hipGetLastError());
  SPL_HIP(hipMemcpyAsync(top + 1, scalars.get() + 1, sizeof(int), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  const int ncolors = top[1] + 1;
  std::vector<int> sizes((size_t)ncolors);
  SPL_HIP(hipMemcpyAsync(sizes.data(), hist.get(), (size_t)ncolors * sizeof(int), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));

  if (d_perm) {
    // a stable sort by colour of keys that stand in ascending vertex order: colour, then ascending index
    DBuf<unsigned long long> keys((size_t)n), alt((size_t)n);
    DBuf<char> temp(radix_sort_u64_temp_bytes(n));
    hipLaunchKernelGGL(color_keys_kernel, dim3(grid_flat(n, grid_cap)), dim3(kRowThreads), 0, s, d_colors, n, keys.get());
    int nbits = 0;
    while ((1ll << nbits) < ncolors) ++nbits;
    const unsigned long long *sorted = radix_sort_u64(keys.get(), alt.get(), n, nbits, temp.get(), s);
    hipLaunchKernelGGL(color_perm_kernel, dim3(grid_flat(n, grid_cap)), dim3(kRowThreads), 0, s, sorted, n, d_perm);
    launches += 2;
    SPL_HIP(hipGetLastError());
    SPL_HIP(hipStreamSynchronize(s));  // the buffers go on return
  }

  int64_t largest = 0, smallest = n;
  for (int c = 0; c < ncolors; ++c) {
    largest = std::max<int64_t>(largest, sizes[(size_t)c]);
    smallest = std::min<int64_t>(smallest, sizes[(size_t)c]);
  }
  if (offsets) {
    int64_t *o = static_cast<int64_t *>(malloc(((size_t)ncolors + 1) * sizeof(int64_t)));
    if (!o) throw std::bad_alloc();
    o[0] = 0;
    for (int c = 0; c < ncolors; ++c) o[c + 1] = o[c] + sizes[(size_t)c];
    *offsets = o;
  }
  info[1] = ncolors;
  info[2] = rounds;
  info[3] = largest;
  info[4] = smallest;
  info[5] = max_degree;
  info[6] = launches;
  return SPL_OK;
}

// out[k] = in[perm[k]], or out[perm[k]] = in[k]; entries of vw doubles moved as bits.  n > 0; enqueues on s
void vector_permute(int64_t n, int vw, const int *d_perm, int inverse, const double *d_in, double *d_out, hipStream_t s) {
  const unsigned grid = grid_flat(n);
  if (vw == 1)
    hipLaunchKernelGGL((vector_permute_kernel<unsigned long long>), dim3(grid), dim3(kRowThreads), 0, s, n, d_perm, inverse,
                       reinterpret_cast<const unsigned long long *>(d_in), reinterpret_cast<unsigned long long *>(d_out));
  else
    hipLaunchKernelGGL((vector_permute_kernel<ulonglong2>), dim3(grid), dim3(kRowThreads), 0, s, n, d_perm, inverse,
                       reinterpret_cast<const ulonglong2 *>(d_in), reinterpret_cast<ulonglong2 *>(d_out));
  SPL_HIP(hipGetLastError());
}

}  // namespace spl

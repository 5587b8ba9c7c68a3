// spmv_panel.hip — workgroup-wide, column-sorted panels: the order-free (1e-10) SpMV mode.
//
// Why: on a matrix without column locality (config C2) the column-blocked lockstep kernel
// (spmv_blocked.hip) is bound by the NUMBER of requests its x gathers send from the CU's vector
// L1 to the L2: one 128-byte line per 8-byte gather, 2.0e8 of them per product, whatever the hit
// rate (profiles/r01_spmv_random_blocked_pmc_detail.txt, profiles/r01_l1_gather_probe.txt).
// Lanes of one load instruction that fall into the same line share one request, so the only way
// to send fewer is to put entries with neighbouring columns next to each other.  Inside one
// wavefront's 1 221-row panel a 128-byte line of x (16 columns) meets 0.04 entries; inside a
// panel that fills the whole LDS (19 532 rows, one per workgroup) it meets 0.63, and sorting the
// panel's entries of a column block BY COLUMN makes 64 neighbouring entries span ~100 lines and
// touch ~47 of them: a quarter fewer requests.
//
// Price: the entries of one row no longer arrive in ascending column order at one wavefront — the
// 16 wavefronts of the workgroup each take every 16th chunk of the column-sorted stream and add
// into the panel's y in LDS with ds_add_f64, so the order in which a row's products are summed is
// the order the hardware happens to execute them in.  Every product a*x and every add is still
// separately rounded; only the ORDER of the adds differs from the reference (Sparse.hs:447-451),
// and may differ from run to run.  north_star's contract is 1e-10 relative on values; this mode
// meets it with rounding-level differences (tests/test_gpu_spmv_panel.py), the column-blocked
// kernel stays available as the reference-order (bit-identical) mode.
//
// Image, built once per matrix in HBM:
//   * rows cut into panels of P rows (P*8 bytes of y = one CU's LDS), columns into index blocks
//     of 2^w columns, w <= 17;
//   * segment (panel, index block): its entries sorted by (column, row) as the packed 32-bit key
//     (local_col << 15 | local_row) + the fp64 value — 12 bytes per entry as before — padded to
//     a multiple of 64 entries with (column 0, row P, value 0): row P is a dummy slot of the LDS
//     image that is never written back, so a whole 64-entry chunk never straddles two blocks and
//     no lane needs a validity test;
//   * segc[panel*nib + ib] = first CHUNK (64 entries) of the segment.
// Kernel: one 16-wavefront workgroup per CU, panels in generations like the lockstep kernel;
// a phase covers K consecutive index blocks (K * 2^w * 8 bytes of x: the window the CUs of an XCD
// gather from together), wavefront i takes chunks i, i+16, ... of the phase, keeps U of them in
// registers, and the stream of the next phase is requested before the barrier that ends this one.
#include "common.hpp"
#include <stdio.h>
#include <atomic>
#include <initializer_list>

namespace spl {

namespace {

constexpr int kRowBits = 15;
constexpr unsigned kRowMask = (1u << kRowBits) - 1u;
constexpr int kPanelWaves = 16;
constexpr int kPanelSlackChunks = 16 * 14 + 16;  // stream loads of a register set may run past the end

inline unsigned blocks_for(int64_t n, int per_block) {
  int64_t b = (n + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : b);
}

// ---- image construction ----------------------------------------------------------------------
template <typename PtrT>
__global__ __launch_bounds__(256) void pnl_count_kernel(int64_t nrows, const PtrT *__restrict__ rowptr,
                                                        const int *__restrict__ colidx, int P, int w,
                                                        int64_t nib, int *__restrict__ segcount) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows) return;
  const int64_t base = (r / P) * nib;
  for (PtrT k = rowptr[r]; k < rowptr[r + 1]; ++k) atomicAdd(&segcount[base + (colidx[k] >> w)], 1);
}

__global__ __launch_bounds__(256) void pnl_chunks_kernel(int64_t nseg, const int *__restrict__ segcount,
                                                         int *__restrict__ chunks, int pair) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nseg) {
    const int c = (segcount[i] + 63) >> 6;
    chunks[i] = pair ? ((c + 1) & ~1) : c;  // paired storage: whole pairs of chunks
  }
}

// paired storage: inside every 128-entry pair of chunks (A, B) the entries are stored A0 B0 A1 B1 ...,
// so that one 16-byte load per lane brings lane l the values (A_l, B_l) and one 8-byte load the keys
__global__ __launch_bounds__(128) void pnl_interleave_kernel(int64_t npairs, unsigned *__restrict__ key,
                                                             double *__restrict__ val) {
  const int64_t pr = blockIdx.x;
  if (pr >= npairs) return;
  const int t = threadIdx.x;
  const int64_t base = pr << 7;
  const unsigned k = key[base + t];
  const double v = val[base + t];
  __syncthreads();
  const int dst = ((t & 63) << 1) | (t >> 6);
  key[base + dst] = k;
  val[base + dst] = v;
}

__global__ __launch_bounds__(256) void pnl_entryptr_kernel(int64_t n, const int *__restrict__ segc,
                                                           int64_t *__restrict__ ptr64) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ptr64[i] = (int64_t)segc[i] << 6;
}

__global__ __launch_bounds__(256) void pnl_padseg_kernel(int64_t n, int last, int *__restrict__ segc, int64_t from) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) segc[from + i] = last;
}

// rounds form: the index block of every unit (pair of chunks) of the paired stream; segments are whole pairs,
// so a unit lies in one block.  Entries behind the last unit stay 0 (they are read, never used).
__global__ __launch_bounds__(256) void pnl_unitblock_kernel(int64_t nseg, int64_t nib, const int *__restrict__ segc,
                                                            int *__restrict__ ublk) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nseg) return;
  const int ib = (int)(i % nib);
  for (int c = segc[i] >> 1, e = segc[i + 1] >> 1; c < e; ++c) ublk[c] = ib;
}

template <typename PtrT>
__global__ __launch_bounds__(256) void pnl_fill_kernel(int64_t nrows, const PtrT *__restrict__ rowptr,
                                                       const int *__restrict__ colidx,
                                                       const double *__restrict__ val, int P, int w,
                                                       int64_t nib, const int *__restrict__ segc,
                                                       int *__restrict__ cursor, unsigned *__restrict__ key,
                                                       double *__restrict__ pval) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrows) return;
  const int64_t base = (r / P) * nib;
  const unsigned lr = (unsigned)(r % P);
  const int wmask = (1 << w) - 1;
  for (PtrT k = rowptr[r]; k < rowptr[r + 1]; ++k) {
    const int c = colidx[k];
    const int64_t seg = base + (c >> w);
    const int64_t pos = ((int64_t)segc[seg] << 6) + atomicAdd(&cursor[seg], 1);
    key[pos] = ((unsigned)(c & wmask) << kRowBits) | lr;
    pval[pos] = val[k];
  }
}

// ---- the kernel ---------------------------------------------------------------------------------
__device__ inline double pnl_gather_issue(const double *p) {
  double v;
  asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
  return v;
}
template <int N>
__device__ inline void pnl_gather_wait(double &v) {
  asm volatile("s_waitcnt vmcnt(%1)" : "+v"(v) : "n"(N) : "memory");
}
__device__ inline void pnl_fold(unsigned id, double prod, double *yp) {
  __builtin_amdgcn_ds_atomic_fadd_f64((__attribute__((address_space(3))) double *)(yp + (id & kRowMask)), prod);
}
// The counted waits behind a burst of gathers, oldest first: gather u of a register set array is awaited while
// First - u younger loads stay in flight (one gather per set), or First - 2u and First - 2u - 1 (two per set, A
// then B).  The immediates are compile-time constants; vmcnt has six bits on gfx9.
template <int First, int U, int u = 0>
__device__ __forceinline__ void pnl_gather_wait_seq(double (&xv)[U]) {
  static_assert(First <= 63 && First - (U - 1) >= 0, "vmcnt immediate out of range");
  if constexpr (u < U) {
    pnl_gather_wait<First - u>(xv[u]);
    pnl_gather_wait_seq<First, U, u + 1>(xv);
  }
}
template <int First, int U, int u = 0>
__device__ __forceinline__ void pnl_gather_wait_seq(double (&xa)[U], double (&xb)[U]) {
  static_assert(First <= 63 && First - (2 * U - 1) >= 0, "vmcnt immediate out of range");
  if constexpr (u < U) {
    pnl_gather_wait<First - 2 * u>(xa[u]);
    pnl_gather_wait<First - 2 * u - 1>(xb[u]);
    pnl_gather_wait_seq<First, U, u + 1>(xa, xb);
  }
}

// ---- the frame every form shares: y of a panel in LDS, the write-back, the rendezvous between generations ----
// the words of PanelImage::arrive
constexpr int kArrive = 0;     // workgroups that have finished a generation
constexpr int kRingError = 1;  // ring form: a bounded wait gave up
constexpr int kLeft = 2;       // rounds form: workgroups that have left the kernel

// ylds[0, P] (P is the dummy row): the panel's rows of y when accumulating into them, else zero
__device__ __forceinline__ void panel_stage_y(double *ylds, const double *y, int64_t row_base, int64_t nrows, int P, bool take_y) {
  for (int i = threadIdx.x; i <= P; i += kPanelWaves * 64)
    ylds[i] = (take_y && i < P && row_base + i < nrows) ? y[row_base + i] : 0.0;
}
// Atomic: the panel's row sums are completed by several workgroups (column slices), global_atomic_add_f64, no return
template <bool Atomic>
__device__ __forceinline__ void panel_store_y(const double *ylds, double *y, int64_t row_base, int64_t nrows, int P) {
  for (int i = threadIdx.x; i < P; i += kPanelWaves * 64)
    if (row_base + i < nrows) {
      if constexpr (Atomic) unsafeAtomicAdd(y + row_base + i, ylds[i]);
      else y[row_base + i] = ylds[i];
    }
}
// re-align the nb workgroups after generation g (bounded, performance only)
__device__ __forceinline__ void panel_rendezvous(unsigned *arrive, int64_t g, int64_t nb) {
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned target = (unsigned)((g + 1) * nb);
    const unsigned long long t0 = wall_clock64();  // 100 MHz
    while (__hip_atomic_load(arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      if (wall_clock64() - t0 > 20000ull) break;  // 200 us: give up, stay correct
      __builtin_amdgcn_s_sleep(8);
    }
  }
  __syncthreads();
}

// A phase of the chunk and the paired form: the K index blocks from ib0 on, of the blocks [.., ibe) this workgroup
// walks.  Boundaries come from the panel's row `sp` of segc (>> Shift: 0 chunks, 1 pairs), clamped to cend, the end
// of the workgroup's stream: [cs, ce) the phase, mid[j] the first unit of block ib0 + j + 1, [ce, cn) the next phase.
// ReadAhead (ibe = nib only: segc carries trailing copies of its last entry): load first, select after — the same
// values, and what the chunk kernels' scalar registers were sized with (profiles/panel_frame_resources.txt).
template <int K>
struct PanelPhaseBounds {
  int cs, ce, cn;
  int mid[K > 1 ? K - 1 : 1];
};
template <int Shift, bool ReadAhead>
__device__ __forceinline__ int panel_boundary(const int *sp, int64_t ib, int64_t ibe, int cend) {
  if constexpr (ReadAhead) { const int t = sp[ib] >> Shift; return (ib < ibe) ? t : cend; }
  else return (ib < ibe) ? sp[ib] >> Shift : cend;
}
template <int K, int Shift, bool ReadAhead>
__device__ __forceinline__ PanelPhaseBounds<K> panel_phase_bounds(const int *sp, int64_t ib0, int64_t ibe, int cend) {
  PanelPhaseBounds<K> b;
#pragma unroll
  for (int j = 0; j + 1 < K; ++j) {
    const int t = ReadAhead ? sp[ib0 + j + 1] >> Shift : panel_boundary<Shift, false>(sp, ib0 + j + 1, ibe, cend);
    b.mid[j] = t < cend ? t : cend;
  }
  b.cs = sp[ib0] >> Shift;
  b.ce = panel_boundary<Shift, ReadAhead>(sp, ib0 + K, ibe, cend);
  b.cn = panel_boundary<Shift, ReadAhead>(sp, ib0 + 2 * K, ibe, cend);
  return b;
}

// One phase, the K index blocks from ib0 on: gather + fold this wavefront's chunks of the phase [cs, ce) held in
// (idC, aC) — chunk u of wavefront i is chunk cs + i + 16 u of the panel's stream — while its chunks of the next
// phase (which starts at ce) are loaded into (idN, aN).  mid[j] is the first chunk of index block
// ib0 + j + 1 (K - 1 of them): the x block a chunk gathers from follows from its position.
// ABL (timing-only ablations, wrong results; refused unless SPL_ALLOW_ABLATION=1): bit 0 every gather reads
// x[lane] (no L2 requests beyond one line), bit 1 no value loads (a = 1), bit 2 no LDS fold
template <int U, int K, int ABL = 0>
__device__ inline void panel_phase(unsigned (&idC)[U], double (&aC)[U], unsigned (&idN)[U], double (&aN)[U],
                                   int cs, const int (&mid)[K > 1 ? K - 1 : 1], int ce, int64_t ib0, int w,
                                   const unsigned *__restrict__ key, const double *__restrict__ val,
                                   const double *__restrict__ x, double *yp, int wave, int nextlen, double &sink,
                                   int64_t dummy) {
  const int lane = threadIdx.x & 63;
  double xv[U];
  const double *xp[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int c = cs + wave + kPanelWaves * u;
    int64_t ib = ib0;
#pragma unroll
    for (int j = 0; j + 1 < K; ++j) ib += (c >= mid[j]) ? 1 : 0;
    const bool ok = c < ce;  // wave-uniform
    xp[u] = x + (ok ? ((ib << w) + (int64_t)(idC[u] >> kRowBits)) : 0);
    if (ABL & 1) xp[u] = x + lane;
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < U; ++u) xv[u] = pnl_gather_issue(xp[u]);  // gathers first ...
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < U; ++u) {  // ... then the next phase's stream, left in flight across the barrier
    // a chunk past the next phase's end would be fetched again by the phase it belongs to: read the
    // (L2-resident) dummy chunk behind the stream instead
    const int c = ce + wave + kPanelWaves * u;
    const int64_t e = (c < ce + nextlen ? ((int64_t)c << 6) : dummy) + lane;  // wave-uniform select
    idN[u] = __builtin_nontemporal_load(key + e);
    if (ABL & 2) aN[u] = 1.0;
    else aN[u] = __builtin_nontemporal_load(val + e);
  }
  __builtin_amdgcn_sched_barrier(0);
  constexpr int Y = ((ABL & 2) ? 2 : 3) * U - 1;  // younger than gather u here: U-1-u gathers + 2U stream loads
  pnl_gather_wait_seq<Y, U>(xv);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (cs + wave + kPanelWaves * u >= ce) break;  // wave-uniform
    if (ABL & 4) sink += aC[u] * xv[u] + (double)(idC[u] & 1u);
    else pnl_fold(idC[u], aC[u] * xv[u], yp);
  }
  for (int c = cs + wave + kPanelWaves * U; c < ce; c += kPanelWaves) {  // tail of an over-long phase
    int64_t ib = ib0;
#pragma unroll
    for (int j = 0; j + 1 < K; ++j) ib += (c >= mid[j]) ? 1 : 0;
    const unsigned id = __builtin_nontemporal_load(key + ((int64_t)c << 6) + lane);
    const double a = __builtin_nontemporal_load(val + ((int64_t)c << 6) + lane);
    pnl_fold(id, a * x[(ib << w) + (int64_t)(id >> kRowBits)], yp);
  }
  __builtin_amdgcn_s_barrier();  // pacing only: no fence, vector memory stays in flight
}

template <int U, int K, int ABL = 0>
__global__ __launch_bounds__(kPanelWaves * 64) void spmv_panel_kernel(
    int64_t nrows, int64_t npanels, int P, int w, int64_t nib, const int *__restrict__ segc,
    const unsigned *__restrict__ key, const double *__restrict__ val, const double *__restrict__ x,
    double *__restrict__ y, int accumulate, unsigned *__restrict__ arrive, int64_t dummy) {
  extern __shared__ __attribute__((aligned(16))) double ylds[];  // P + 1 doubles
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nb = gridDim.x;
  const int64_t ngen = (npanels + nb - 1) / nb;
  const int64_t nph = (nib + K - 1) / K;
  for (int64_t g = 0; g < ngen; ++g) {
    const int64_t p = g * nb + blockIdx.x;
    if (p >= npanels) break;  // only in the last generation: no rendezvous follows
    const int64_t row_base = p * P;
    const int *sp = segc + p * nib;  // segc carries K + 1 trailing copies of its last entry
    const int c0 = sp[0];
    unsigned idA[U], idB[U];
    double aA[U], aB[U];
    double sink = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) {  // prologue: this wavefront's first chunks of phase 0
      const int c = c0 + wave + kPanelWaves * u;
      const int64_t k = (c < (K < nib ? sp[K] : sp[nib]) ? ((int64_t)c << 6) : dummy) + lane;
      idA[u] = __builtin_nontemporal_load(key + k);
      aA[u] = __builtin_nontemporal_load(val + k);
    }
    panel_stage_y(ylds, y, row_base, nrows, P, accumulate);
    __syncthreads();
    const int cend = sp[nib];
    for (int64_t ph = 0; ph < nph; ph += 2) {  // the two register sets take turns
      {
        const PanelPhaseBounds<K> b = panel_phase_bounds<K, 0, true>(sp, ph * K, nib, cend);
        panel_phase<U, K, ABL>(idA, aA, idB, aB, b.cs, b.mid, b.ce, ph * K, w, key, val, x, ylds, wave, b.cn - b.ce, sink, dummy);
      }
      if (ph + 1 < nph) {
        const PanelPhaseBounds<K> b = panel_phase_bounds<K, 0, true>(sp, (ph + 1) * K, nib, cend);
        panel_phase<U, K, ABL>(idB, aB, idA, aA, b.cs, b.mid, b.ce, (ph + 1) * K, w, key, val, x, ylds, wave, b.cn - b.ce, sink, dummy);
      }
    }
    if (ABL && sink == 1.2345e-300) ylds[0] = sink;  // keeps the ablated arithmetic alive
    __syncthreads();  // every wavefront's LDS adds are done (s_barrier above does not wait for lgkmcnt)
    panel_store_y<false>(ylds, y, row_base, nrows, P);
    if (g + 1 < ngen) panel_rendezvous(arrive + kArrive, g, nb);
  }
}


// ---- paired form ------------------------------------------------------------------------------------
// Same two-stage schedule on the paired storage: a wavefront's unit of work is a PAIR of chunks, read
// with one 8-byte key load and one 16-byte value load per lane (half the stream instructions for the
// same bytes: the HBM stream of a CU runs closer to its peak with fewer, wider requests in flight —
// tools/probe/tcp_mix_probe.hip S rows), gathered with two instructions (chunk A, chunk B: each a run
// of 64 column-sorted entries as before) and folded with two.  All units here are pairs.
typedef unsigned pnl_u2 __attribute__((ext_vector_type(2)));
typedef double pnl_d2 __attribute__((ext_vector_type(2)));

template <int U, int K>
__device__ inline void panelw_phase(pnl_u2 (&idC)[U], pnl_d2 (&aC)[U], pnl_u2 (&idN)[U], pnl_d2 (&aN)[U], int cs,
                                    const int (&mid)[K > 1 ? K - 1 : 1], int ce, int64_t ib0, int w,
                                    const pnl_u2 *__restrict__ key2, const pnl_d2 *__restrict__ val2,
                                    const double *__restrict__ x, double *yp, int wave, int cn, int64_t dummy) {
  const int lane = threadIdx.x & 63;
  double xa[U], xb[U];
  const double *pa[U], *pb[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int c = cs + wave + kPanelWaves * u;
    int64_t ib = ib0;
#pragma unroll
    for (int j = 0; j + 1 < K; ++j) ib += (c >= mid[j]) ? 1 : 0;
    const bool ok = c < ce;  // wave-uniform
    pa[u] = x + (ok ? ((ib << w) + (int64_t)(idC[u].x >> kRowBits)) : 0);
    pb[u] = x + (ok ? ((ib << w) + (int64_t)(idC[u].y >> kRowBits)) : 0);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < U; ++u) {  // gathers first ...
    xa[u] = pnl_gather_issue(pa[u]);
    xb[u] = pnl_gather_issue(pb[u]);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < U; ++u) {  // ... then the next phase's stream, left in flight across the barrier
    // a unit past the next phase's end [ce, cn) would be fetched again by the phase it belongs to: read
    // the (L2-resident) dummy unit instead, so that U may exceed the mean count without costing HBM bytes
    const int c = ce + wave + kPanelWaves * u;
    const int64_t e = (c < cn ? ((int64_t)c << 6) : dummy) + lane;  // wave-uniform select
    idN[u] = __builtin_nontemporal_load(key2 + e);
    aN[u] = __builtin_nontemporal_load(val2 + e);
  }
  __builtin_amdgcn_sched_barrier(0);
  // younger than gather j (j = 2u for A, 2u + 1 for B) here: 2U-1-j gathers + 2U stream loads
  pnl_gather_wait_seq<4 * U - 1, U>(xa, xb);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (cs + wave + kPanelWaves * u >= ce) break;  // wave-uniform
    pnl_fold(idC[u].x, aC[u].x * xa[u], yp);
    pnl_fold(idC[u].y, aC[u].y * xb[u], yp);
  }
  for (int c = cs + wave + kPanelWaves * U; c < ce; c += kPanelWaves) {  // tail of an over-long phase
    int64_t ib = ib0;
#pragma unroll
    for (int j = 0; j + 1 < K; ++j) ib += (c >= mid[j]) ? 1 : 0;
    const pnl_u2 id = __builtin_nontemporal_load(key2 + ((int64_t)c << 6) + lane);
    const pnl_d2 a = __builtin_nontemporal_load(val2 + ((int64_t)c << 6) + lane);
    pnl_fold(id.x, a.x * x[(ib << w) + (int64_t)(id.x >> kRowBits)], yp);
    pnl_fold(id.y, a.y * x[(ib << w) + (int64_t)(id.y >> kRowBits)], yp);
  }
  __builtin_amdgcn_s_barrier();  // pacing only
}

// Column slices (round 3): with `ns` > 1 the index blocks are dealt to ns slices and workgroup b works on slice
// b % ns (workgroups go round-robin to the 8 XCDs, so with ns = 8 a slice is what ONE XCD's L2 has to hold) of
// panel slot b / ns: a panel's row sums are then completed by ns workgroups, which add their parts into y with
// global_atomic_add_f64 (y zeroed by the launcher unless accumulating).  Why: every XCD that works on a panel
// pulls the x lines that panel touches through its own L2 once per generation, so x costs (rows / (panels per
// generation of one XCD * P)) * 8 bytes * ncols of fabric traffic per product — a row block too short to give
// every CU a full-height panel (a rank's block at N = 4, 8) would otherwise pay with short panels (fewer lanes
// per line of x, more passes over x): 640 MB of x for 300 MB of matrix at N = 8.  With slices the panels keep
// the full LDS height and each XCD reads an eighth of x per generation.
template <int U, int K>
__global__ __launch_bounds__(kPanelWaves * 64) void spmv_panelw_kernel(
    int64_t nrows, int64_t npanels, int P, int w, int64_t nib, const int *__restrict__ segc,
    const unsigned *__restrict__ key, const double *__restrict__ val, const double *__restrict__ x,
    double *__restrict__ y, int accumulate, unsigned *__restrict__ arrive, int64_t dummy, int ns) {
  extern __shared__ __attribute__((aligned(16))) double ylds[];  // P + 1 doubles
  const pnl_u2 *key2 = reinterpret_cast<const pnl_u2 *>(key);
  const pnl_d2 *val2 = reinterpret_cast<const pnl_d2 *>(val);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t ppg = gridDim.x / ns;          // panels per generation
  const int slice = (int)(blockIdx.x % ns);
  const int64_t slot = blockIdx.x / ns;
  if (slot >= ppg) return;                      // grid not a multiple of ns: the extra workgroups idle
  const int64_t nb = ppg * ns;                  // workgroups that take part in the rendezvous
  const int64_t ngen = (npanels + ppg - 1) / ppg;
  const int64_t ibs = nib * slice / ns, ibe = nib * (slice + 1) / ns;  // this slice's index blocks
  const int64_t nph = (ibe - ibs + K - 1) / K;
  for (int64_t g = 0; g < ngen; ++g) {
    const int64_t p = g * ppg + slot;
    if (p >= npanels) break;
    const int64_t row_base = p * P;
    const int *sp = segc + p * nib;  // in chunks; every boundary is even (whole pairs)
    const int c0 = sp[ibs] >> 1;
    const int cend = sp[ibe] >> 1;
    const int c1 = (ibs + K < ibe ? sp[ibs + K] >> 1 : cend);
    pnl_u2 idA[U], idB[U];
    pnl_d2 aA[U], aB[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = c0 + wave + kPanelWaves * u;
      const int64_t k = (c < c1 ? ((int64_t)c << 6) : dummy) + lane;
      idA[u] = __builtin_nontemporal_load(key2 + k);
      aA[u] = __builtin_nontemporal_load(val2 + k);
    }
    panel_stage_y(ylds, y, row_base, nrows, P, ns == 1 && accumulate);
    __syncthreads();
    for (int64_t ph = 0; ph < nph; ph += 2) {  // the two register sets take turns
      {
        const PanelPhaseBounds<K> b = panel_phase_bounds<K, 1, false>(sp, ibs + ph * K, ibe, cend);
        panelw_phase<U, K>(idA, aA, idB, aB, b.cs, b.mid, b.ce, ibs + ph * K, w, key2, val2, x, ylds, wave, b.cn, dummy);
      }
      if (ph + 1 < nph) {
        const PanelPhaseBounds<K> b = panel_phase_bounds<K, 1, false>(sp, ibs + (ph + 1) * K, ibe, cend);
        panelw_phase<U, K>(idB, aB, idA, aA, b.cs, b.mid, b.ce, ibs + (ph + 1) * K, w, key2, val2, x, ylds, wave, b.cn, dummy);
      }
    }
    __syncthreads();
    if (ns == 1) panel_store_y<false>(ylds, y, row_base, nrows, P);
    else panel_store_y<true>(ylds, y, row_base, nrows, P);
    if (g + 1 < ngen) panel_rendezvous(arrive + kArrive, g, nb);
  }
}

// ---- rounds form: fixed-length rounds instead of index-block phases ---------------------------------------
// The paired form ties the barrier-to-barrier phase to index-block boundaries: a phase of K blocks holds
// 16 U units only on average, and on C2 69 % of the phases are a unit or two longer, which sends one to three
// wavefronts through the un-pipelined tail loop while the others wait at the barrier: some wavefront of a CU is
// in that loop during 27 % of the launch (profiles/panel_rounds_before.txt; the tail's load is awaited with
// vmcnt(0), behind the whole stream of the next phase).  And the register sets cannot be chosen freely: fewer
// than the mean phase needs means longer tails, more means dummy loads.  Nothing in the result needs either:
// the block of a unit follows from its position,
// the barrier is pacing only.  Here a panel's paired stream is one sequence of units and a round is exactly
// 16 U consecutive units (only a panel's last round is shorter): wavefront i takes units i, i + 16, ... of the
// round into its U register sets, the next round's units are requested before the barrier, and the block of
// every unit comes from a per-unit table (PanelImage::ublk, 4 bytes per 1 536 of stream) through the scalar
// cache — a vector load would sit on vmcnt in front of the gathers (ring_sload below).  No tail loop, no
// dummy units except behind a panel's end, and any segment size works (empty, shorter or longer than a round).
// Measured on C2: 4 register sets 0.82 ms (the paired form's best, 5 sets x 2 blocks: 0.91 ms), 3: 0.85, 5: 0.90,
// 6: 0.95 (profiles/panel_rounds_bench.json).  Column slices stay with the paired form.
template <int U>
__device__ inline void panelq_blocks_issue(int (&ib)[U], const int *p) {  // ib[u] = p[16 u], not awaited
#pragma unroll
  for (int u = 0; u < U; ++u) asm volatile("s_load_dword %0, %1, %2" : "=s"(ib[u]) : "s"(p), "n"(kPanelWaves * 4 * u) : "memory");
}
template <int U>
__device__ inline void panelq_blocks_wait(int (&ib)[U]) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
  for (int u = 0; u < U; ++u) asm volatile("" : "+s"(ib[u]));  // every use stays behind the wait
}

// One round: gather + fold this wavefront's units m0 + wave + 16 u (u < U; panel-relative, the panel has nu)
// held in (idC, aC, ibC) while its units of the next round are loaded into (idN, aN, ibN).
template <int U>
__device__ inline void panelq_round(pnl_u2 (&idC)[U], pnl_d2 (&aC)[U], int (&ibC)[U], pnl_u2 (&idN)[U], pnl_d2 (&aN)[U],
                                    int (&ibN)[U], int m0, int nu, int c0, int w, const pnl_u2 *__restrict__ key2,
                                    const pnl_d2 *__restrict__ val2, const int *__restrict__ ublk,
                                    const double *__restrict__ x, double *yp, int wave, int64_t dummy) {
  const int lane = threadIdx.x & 63;
  double xa[U], xb[U];
  const double *pa[U], *pb[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const bool ok = m0 + wave + kPanelWaves * u < nu;  // wave-uniform; false only in a panel's last round
    const int64_t xo = (int64_t)ibC[u] << w;
    pa[u] = x + (ok ? (xo + (int64_t)(idC[u].x >> kRowBits)) : 0);
    pb[u] = x + (ok ? (xo + (int64_t)(idC[u].y >> kRowBits)) : 0);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < U; ++u) {  // gathers first ...
    xa[u] = pnl_gather_issue(pa[u]);
    xb[u] = pnl_gather_issue(pb[u]);
  }
  __builtin_amdgcn_sched_barrier(0);
  const int mn = m0 + kPanelWaves * U + wave;
#pragma unroll
  for (int u = 0; u < U; ++u) {  // ... then the next round's stream, left in flight across the barrier
    const int m = mn + kPanelWaves * u;
    const int64_t e = (m < nu ? ((int64_t)(c0 + m) << 6) : dummy) + lane;  // behind the panel: the L2-resident dummy unit
    idN[u] = __builtin_nontemporal_load(key2 + e);
    aN[u] = __builtin_nontemporal_load(val2 + e);
  }
  panelq_blocks_issue<U>(ibN, ublk + c0 + mn);  // the table carries slack behind the last unit
  __builtin_amdgcn_sched_barrier(0);
  // younger than gather j (j = 2u for A, 2u + 1 for B) here: 2U-1-j gathers + 2U stream loads
  pnl_gather_wait_seq<4 * U - 1, U>(xa, xb);
  panelq_blocks_wait<U>(ibN);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    if (m0 + wave + kPanelWaves * u >= nu) break;  // wave-uniform
    pnl_fold(idC[u].x, aC[u].x * xa[u], yp);
    pnl_fold(idC[u].y, aC[u].y * xb[u], yp);
  }
  __builtin_amdgcn_s_barrier();  // pacing only: no fence, vector memory stays in flight
}

// arrive[kArrive]: rendezvous between generations, arrive[kLeft]: workgroups that have left.  The last one to leave
// puts both back to zero, so a stream of launches holds nothing but this kernel (the other forms clear
// arrive[kArrive] with a memset in front of every launch).
// meet = 0: no rendezvous, a workgroup starts its next panel at once.  The rendezvous is pacing only (it keeps an
// XCD's CUs in the same x window); on C2 a workgroup waits 20 us of an 817 us launch there for the slowest of 256
// (profiles/panel_claims_before.txt), and without it a step is 2.3 % shorter.  Which is better depends on the
// matrix, so the build's one-time timing decides (tune_panel_plan); an explicit request keeps the rendezvous.
template <int U>
__global__ __launch_bounds__(kPanelWaves * 64) void spmv_panelq_kernel(
    int64_t nrows, int64_t npanels, int P, int w, int64_t nib, const int *__restrict__ segc,
    const int *__restrict__ ublk, const unsigned *__restrict__ key, const double *__restrict__ val,
    const double *__restrict__ x, double *__restrict__ y, int accumulate, unsigned *__restrict__ arrive,
    int64_t dummy, int meet) {
  static_assert(U >= 3 && U <= 6, "register sets per wavefront");
  extern __shared__ __attribute__((aligned(16))) double ylds[];  // P + 1 doubles
  const pnl_u2 *key2 = reinterpret_cast<const pnl_u2 *>(key);
  const pnl_d2 *val2 = reinterpret_cast<const pnl_d2 *>(val);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nb = gridDim.x;
  const int64_t ngen = (npanels + nb - 1) / nb;
  constexpr int kRound = kPanelWaves * U;
  for (int64_t g = 0; g < ngen; ++g) {
    const int64_t p = g * nb + blockIdx.x;
    if (p >= npanels) break;  // only in the last generation: no rendezvous follows
    const int64_t row_base = p * P;
    const int c0 = segc[p * nib] >> 1;  // in units; every segment boundary is a whole pair
    const int nu = (segc[(p + 1) * nib] >> 1) - c0;
    pnl_u2 idA[U], idB[U];
    pnl_d2 aA[U], aB[U];
    int ibA[U], ibB[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {  // prologue: this wavefront's units of round 0
      const int m = wave + kPanelWaves * u;
      const int64_t k = (m < nu ? ((int64_t)(c0 + m) << 6) : dummy) + lane;
      idA[u] = __builtin_nontemporal_load(key2 + k);
      aA[u] = __builtin_nontemporal_load(val2 + k);
    }
    panelq_blocks_issue<U>(ibA, ublk + c0 + wave);
    panelq_blocks_wait<U>(ibA);
    panel_stage_y(ylds, y, row_base, nrows, P, accumulate);
    __syncthreads();
    for (int m0 = 0; m0 < nu; m0 += 2 * kRound) {
      panelq_round<U>(idA, aA, ibA, idB, aB, ibB, m0, nu, c0, w, key2, val2, ublk, x, ylds, wave, dummy);
      if (m0 + kRound < nu)
        panelq_round<U>(idB, aB, ibB, idA, aA, ibA, m0 + kRound, nu, c0, w, key2, val2, ublk, x, ylds, wave, dummy);
    }
    __syncthreads();  // every wavefront's LDS adds are done (s_barrier above does not wait for lgkmcnt)
    panel_store_y<false>(ylds, y, row_base, nrows, P);
    if (g + 1 < ngen && meet) panel_rendezvous(arrive + kArrive, g, nb);
  }
  // leave: whoever arrives last knows that nobody will touch the rendezvous word again in this launch
  if (threadIdx.x == 0 &&
      __hip_atomic_fetch_add(arrive + kLeft, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)nb - 1u) {
    __hip_atomic_store(arrive + kArrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(arrive + kLeft, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- ring form (round 3): loader wavefronts + gather wavefronts ---------------------------------------
// What the probes say (tools/probe/lds_dma_mix_probe.hip, profiles/r03_tcp_mix_lds_dma.txt): when every
// wavefront carries both the HBM stream and the L2 gathers, the two times ADD (vmcnt retires in order, so a
// wavefront's gathers wait behind its own stream loads, and the stream arrives in bursts of a whole phase);
// when a few wavefronts do nothing but keep ~32 KiB of 16-byte stream loads in flight and the others do
// nothing but gather, the mix takes 0.82x the sum.  LDS-DMA for the stream does not help (it adds up like
// the register loads do, and more).  So: NL loader wavefronts stream the paired image into registers (D
// units of 1.5 KiB each in flight per loader) and hand every unit through a 1.5 KiB slot in LDS to one of
// its R = (16 - NL) / NL gather wavefronts, which keeps GD units (2 GD gather instructions) in flight and
// folds with ds_add_f64 as before.  The panel keeps (almost) the whole LDS: the hand-over slots are NL * S
// units (6 KiB for NL = 4, S = 1).
//   slot header {seq, ib}: seq = t + 1 while the loader's t-th unit waits in the slot, 0 = free.  LDS
//   operations of one wavefront execute in program order, so data written before the header is visible
//   to whoever sees the header, and a header cleared after the reads have returned frees the slot.
//   Phase barriers (pacing only, as in the other forms): a gather wavefront crosses barrier p before it
//   gathers its first unit beyond phase p (it has taken that unit out of its slot by then); a loader
//   crosses it once each of its gather wavefronts has been handed a unit beyond phase p (its last R
//   deliveries are all beyond p), or at the end of the stream.  Nobody waits at a barrier for something
//   that only a wavefront behind that barrier can provide.  Every wait is bounded (spin limit -> error
//   word, results then wrong but the grid drains).
constexpr int kRingUnitBytes = 1536;
constexpr unsigned kRingSpinLimit = 1u << 22;

// a wave-uniform int through the scalar cache: a vector load here would sit on vmcnt behind the loader's stream
__device__ inline int ring_sload(const int *p) {
  int v;
  asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
  return v;
}

// the loader's stream loads, outside the compiler's wait bookkeeping (it drains vmcnt to 0 at every loop
// header): issued here, awaited with a counted vmcnt by ring_stream_wait
__device__ inline void ring_stream_issue(pnl_u2 &k, pnl_d2 &v, const pnl_u2 *kp, const pnl_d2 *vp) {
  asm volatile("global_load_dwordx2 %0, %1, off nt" : "=v"(k) : "v"(kp) : "memory");
  asm volatile("global_load_dwordx4 %0, %1, off nt" : "=v"(v) : "v"(vp) : "memory");
}
template <int N>
__device__ inline void ring_stream_wait(pnl_u2 &k, pnl_d2 &v) {
  asm volatile("s_waitcnt vmcnt(%2)" : "+v"(k), "+v"(v) : "n"(N) : "memory");
}

__device__ inline void ring_fail(unsigned *err) { __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <int NL, int D, int GD, int K, int S>
__global__ __launch_bounds__(kPanelWaves * 64) void spmv_panelr_kernel(
    int64_t nrows, int64_t npanels, int P, int w, int64_t nib, const int *__restrict__ segc,
    const unsigned *__restrict__ key, const double *__restrict__ val, const double *__restrict__ x,
    double *__restrict__ y, int accumulate, unsigned *__restrict__ arrive, int64_t dummy) {
  extern __shared__ __attribute__((aligned(16))) double ylds[];  // P + 1 doubles, then the slots, then their headers
  constexpr int R = (kPanelWaves - NL) / NL;
  static_assert(NL * (R + 1) == kPanelWaves, "NL must divide 16");
  const pnl_u2 *key2 = reinterpret_cast<const pnl_u2 *>(key);
  const pnl_d2 *val2 = reinterpret_cast<const pnl_d2 *>(val);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // explicit LDS pointers: a generic pointer would turn every access into a flat_ instruction (vmcnt + lgkmcnt)
  typedef __attribute__((address_space(3))) char lds_char;
  typedef __attribute__((address_space(3))) pnl_u2 lds_u2;
  typedef __attribute__((address_space(3))) pnl_d2 lds_d2;
  lds_char *ring = (lds_char *)ylds + ((((size_t)P + 1) * sizeof(double) + 15) & ~(size_t)15);
  volatile lds_u2 *hdr = (volatile lds_u2 *)(ring + NL * S * kRingUnitBytes);
  const int64_t nb = gridDim.x;
  const int64_t ngen = (npanels + nb - 1) / nb;
  const int nph = (int)((nib + K - 1) / K);
  for (int64_t g = 0; g < ngen; ++g) {
    const int64_t p = g * nb + blockIdx.x;
    if (p >= npanels) break;
    const int64_t row_base = p * P;
    const int *sp = segc + p * nib;  // in chunks; every boundary is even (whole pairs)
    const int c0 = sp[0] >> 1;
    const int nu = (sp[nib] >> 1) - c0;  // units (pairs of chunks) of this panel
    panel_stage_y(ylds, y, row_base, nrows, P, accumulate);
    if (threadIdx.x < NL * S) { pnl_u2 z = {0u, 0u}; hdr[threadIdx.x] = z; }
    __syncthreads();
    int bar_done = 0;
    if (wave < NL) {
      // ---- loader ----
      const int L = wave;
      const int nt = nu > L ? (nu - L + NL - 1) / NL : 0;
      pnl_u2 kr[D];
      pnl_d2 vr[D];
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int m = L + NL * d;
        const int64_t e = (m < nu ? ((int64_t)(c0 + m) << 6) : dummy) + lane;
        ring_stream_issue(kr[d], vr[d], key2 + e, val2 + e);
      }
      int ibc = 0;
      int hist[R];  // phases of the last R units handed over, oldest first
#pragma unroll
      for (int r = 0; r < R; ++r) hist[r] = 0;
      for (int t0 = 0; t0 < nt; t0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const int t = t0 + d;
          if (t >= nt) break;  // wave-uniform
          const int c = c0 + L + NL * t;
          while (ibc + 1 < (int)nib && c >= (ring_sload(sp + ibc + 1) >> 1)) ++ibc;
          const int sl = L * S + (S > 1 ? t % S : 0);
          unsigned spins = 0;
          while (__builtin_amdgcn_readfirstlane(hdr[sl].x) != 0u) {  // the slot still holds an earlier unit
            __builtin_amdgcn_s_sleep(1);
            if (++spins > kRingSpinLimit) { ring_fail(arrive + kRingError); break; }
          }
          lds_char *slot = ring + sl * kRingUnitBytes;
          ring_stream_wait<2 * (D - 1)>(kr[d], vr[d]);  // D - 1 younger units stay in flight
          ((lds_u2 *)slot)[lane] = kr[d];
          ((lds_d2 *)(slot + 512))[lane] = vr[d];
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          if (lane == 0) { pnl_u2 h = {(unsigned)(t + 1), (unsigned)ibc}; hdr[sl] = h; }
          {  // refill this register set: the unit D places further down this loader's sequence
            const int m = L + NL * (t + D);
            const int64_t e = (m < nu ? ((int64_t)(c0 + m) << 6) : dummy) + lane;
            ring_stream_issue(kr[d], vr[d], key2 + e, val2 + e);
          }
#pragma unroll
          for (int r = 0; r + 1 < R; ++r) hist[r] = hist[r + 1];
          hist[R - 1] = ibc / K;
          while (bar_done < hist[0]) { __builtin_amdgcn_s_barrier(); ++bar_done; }
        }
      }
    } else {
      // ---- gather wavefront ----
      const int j = wave - NL;
      const int L = j % NL, q = j / NL;
      const int nt = nu > L ? (nu - L + NL - 1) / NL : 0;  // units of my loader; mine are q, q + R, ...
      pnl_u2 id[GD];
      pnl_d2 a[GD];
      double xa[GD], xb[GD];
      bool first = true;
      int t = q;
      int live = 0;  // units issued and not yet folded at loop exit
      while (t < nt) {
        live = 0;
#pragma unroll
        for (int u = 0; u < GD; ++u) {
          if (t >= nt) break;  // wave-uniform
          if (!first) {
            pnl_gather_wait<2 * (GD - 1) + 1>(xa[u]);
            pnl_gather_wait<2 * (GD - 1)>(xb[u]);
            pnl_fold(id[u].x, a[u].x * xa[u], ylds);
            pnl_fold(id[u].y, a[u].y * xb[u], ylds);
          }
          const int sl = L * S + (S > 1 ? t % S : 0);
          unsigned spins = 0;
          pnl_u2 h;
          for (;;) {
            h = hdr[sl];
            if (__builtin_amdgcn_readfirstlane(h.x) == (unsigned)(t + 1)) break;
            __builtin_amdgcn_s_sleep(1);
            if (++spins > kRingSpinLimit) { ring_fail(arrive + kRingError); break; }
          }
          const int ib = __builtin_amdgcn_readfirstlane(h.y);
          const lds_char *slot = ring + sl * kRingUnitBytes;
          id[u] = ((const lds_u2 *)slot)[lane];
          a[u] = ((const lds_d2 *)(slot + 512))[lane];
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(id[u]), "+v"(a[u]) : : "memory");
          if (lane == 0) { pnl_u2 z = {0u, 0u}; hdr[sl] = z; }
          const int ph = ib / K;
          while (bar_done < ph) { __builtin_amdgcn_s_barrier(); ++bar_done; }
          const double *xw = x + ((int64_t)ib << w);
          xa[u] = pnl_gather_issue(xw + (id[u].x >> kRowBits));
          xb[u] = pnl_gather_issue(xw + (id[u].y >> kRowBits));
          t += R;
          ++live;
        }
        if (live == GD) first = false;
        else break;
      }
      // drain: everything still in flight (the last full round's units that were not re-used + the partial round)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int u = 0; u < GD; ++u) {
        const bool pending = first ? (u < live) : true;  // after a full round every set holds an unfolded unit
        if (pending) {
          pnl_gather_wait<0>(xa[u]);
          pnl_gather_wait<0>(xb[u]);
          pnl_fold(id[u].x, a[u].x * xa[u], ylds);
          pnl_fold(id[u].y, a[u].y * xb[u], ylds);
        }
      }
    }
    while (bar_done < nph) { __builtin_amdgcn_s_barrier(); ++bar_done; }
    __syncthreads();
    panel_store_y<false>(ylds, y, row_base, nrows, P);
    if (g + 1 < ngen) panel_rendezvous(arrive + kArrive, g, nb);
  }
}

}  // namespace

void build_panel_image(Matrix *m, int P, int w, int pair, hipStream_t s) {
  auto b = std::make_unique<PanelImage>();
  b->P = P;
  b->w = w;
  b->npanels = (m->nrows_local + P - 1) / P;
  b->nib = (m->ncols + (1LL << w) - 1) >> w;
  if (b->nib < 1) b->nib = 1;
  const int64_t nseg = b->npanels * b->nib;
  constexpr int kSegPad = 10;  // trailing copies of the last boundary (the kernel peeks 2 K blocks ahead)
  DBuf<int> counts((size_t)nseg + 1);
  DBuf<int> chunks((size_t)nseg + 1);
  DBuf<int64_t> off64((size_t)nseg + 2);
  b->segc.alloc((size_t)nseg + 1 + kSegPad);
  SPL_HIP(hipMemsetAsync(counts.get(), 0, ((size_t)nseg + 1) * sizeof(int), s));
  const unsigned grid = blocks_for(m->nrows_local, 256);
  if (m->nrows_local > 0) {
    if (m->rowptr.get())
      hipLaunchKernelGGL(pnl_count_kernel<int>, dim3(grid), dim3(256), 0, s, m->nrows_local, m->rowptr.get(),
                         m->colidx.get(), P, w, b->nib, counts.get());
    else
      hipLaunchKernelGGL(pnl_count_kernel<int64_t>, dim3(grid), dim3(256), 0, s, m->nrows_local,
                         m->rowptr64.get(), m->colidx.get(), P, w, b->nib, counts.get());
  }
  hipLaunchKernelGGL(pnl_chunks_kernel, dim3(blocks_for(nseg, 256)), dim3(256), 0, s, nseg, counts.get(),
                     chunks.get(), pair);
  exclusive_scan_i32_to_i64(chunks.get(), off64.get(), nseg, s);
  int64_t nchunks = 0;
  SPL_HIP(hipMemcpyAsync(&nchunks, off64.get() + nseg, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  if (nchunks >= (int64_t)0x7fffffff - kPanelSlackChunks) throw DeviceError{SPL_ERROR_index_overflow};
  b->nchunks = nchunks;
  narrow_i64_to_i32(off64.get(), b->segc.get(), nseg + 1, s);
  hipLaunchKernelGGL(pnl_padseg_kernel, dim3(1), dim3(256), 0, s, (int64_t)kSegPad, (int)nchunks, b->segc.get(),
                     nseg + 1);
  const size_t entries = ((size_t)nchunks + kPanelSlackChunks) * 64;
  b->key.alloc(entries);
  b->val.alloc(entries);
  // padding: column 0 of the block, the dummy row P, value 0
  SPL_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(b->key.get()), P, entries, s));
  SPL_HIP(hipMemsetAsync(b->val.get(), 0, entries * sizeof(double), s));
  b->arrive.alloc(4);  // [0] generation rendezvous, [1] ring form: a bounded wait gave up, [2] rounds form: workgroups gone
  SPL_HIP(hipMemsetAsync(b->arrive.get(), 0, 4 * sizeof(unsigned), s));
  SPL_HIP(hipMemsetAsync(counts.get(), 0, ((size_t)nseg + 1) * sizeof(int), s));
  if (m->nrows_local > 0) {
    if (m->rowptr.get())
      hipLaunchKernelGGL(pnl_fill_kernel<int>, dim3(grid), dim3(256), 0, s, m->nrows_local, m->rowptr.get(),
                         m->colidx.get(), m->val.get(), P, w, b->nib, b->segc.get(), counts.get(), b->key.get(),
                         b->val.get());
    else
      hipLaunchKernelGGL(pnl_fill_kernel<int64_t>, dim3(grid), dim3(256), 0, s, m->nrows_local,
                         m->rowptr64.get(), m->colidx.get(), m->val.get(), P, w, b->nib, b->segc.get(),
                         counts.get(), b->key.get(), b->val.get());
  }
  // cursor slots were handed out in arbitrary order: sort every padded segment by (column, row)
  hipLaunchKernelGGL(pnl_entryptr_kernel, dim3(blocks_for(nseg + 1, 256)), dim3(256), 0, s, nseg + 1,
                     b->segc.get(), off64.get());
  segmented_sort_pairs_u32(off64.get(), nseg, b->key.get(), b->val.get(), s);
  b->pair = pair ? 1 : 0;
  if (pair && nchunks > 0)
    hipLaunchKernelGGL(pnl_interleave_kernel, dim3((unsigned)(nchunks / 2)), dim3(128), 0, s, nchunks / 2,
                       b->key.get(), b->val.get());
  if (pair) {  // rounds form: the index block of every unit; the slack behind the last one is read, never used
    const size_t units = (size_t)(nchunks / 2) + kPanelSlackChunks;
    b->ublk.alloc(units);
    SPL_HIP(hipMemsetAsync(b->ublk.get(), 0, units * sizeof(int), s));
    hipLaunchKernelGGL(pnl_unitblock_kernel, dim3(blocks_for(nseg, 256)), dim3(256), 0, s, nseg, b->nib,
                       b->segc.get(), b->ublk.get());
  }
  SPL_HIP(hipStreamSynchronize(s));
  delete m->panel;
  m->panel = b.release();
}

// ---- the launch plan --------------------------------------------------------------------------------
// One kernel launcher for every form: the dynamic-LDS attribute is per kernel and per device.
template <auto Kernel, class... Args>
static void launch_panel_kernel(int device, unsigned grid, size_t lds, hipStream_t s, Args... args) {
  static std::atomic<uint64_t> set_{0};  // bit d: attribute set on device d
  if (!(set_.load(std::memory_order_acquire) >> (device & 63) & 1u)) {
    SPL_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024));
    set_.fetch_or(1ull << (device & 63), std::memory_order_release);
  }
  hipLaunchKernelGGL(Kernel, dim3(grid), dim3(kPanelWaves * 64), lds, s, args...);
}

size_t panel_ring_lds_bytes(int P, int nl, int slots) {
  return ((((size_t)P + 1) * sizeof(double) + 15) & ~(size_t)15) + (size_t)nl * slots * (kRingUnitBytes + 8);
}

namespace {

constexpr size_t kPanelLdsLimit = 160 * 1024;

struct PanelLaunchArgs { const Matrix *m; const PanelImage *b; unsigned nb; const double *x; double *y; int accumulate; hipStream_t s; };

inline size_t panel_lds_bytes(const PanelImage *b) { return ((size_t)b->P + 1) * sizeof(double); }
inline void clear_word(const PanelLaunchArgs &a, int word) {
  SPL_HIP(hipMemsetAsync(a.b->arrive.get() + word, 0, sizeof(unsigned), a.s));
}
// the chunk, paired and ring kernels take the same arguments up to `arrive`; tail: the dummy unit behind the stream, ...
template <auto Kernel, class... Tail>
void launch_on_image(const PanelLaunchArgs &a, size_t lds, Tail... tail) {
  const PanelImage *b = a.b;
  launch_panel_kernel<Kernel>(a.m->device, a.nb, lds, a.s, a.m->nrows_local, b->npanels, b->P, b->w, b->nib, b->segc.get(),
                              b->key.get(), b->val.get(), a.x, a.y, a.accumulate, b->arrive.get(), tail...);
}
// what each form puts on the stream besides its kernel is written here, once per form
template <int U, int K, int ABL>
void run_chunk(const PanelLaunchArgs &a, const PanelPlan &) {
  clear_word(a, kArrive);
  launch_on_image<&spmv_panel_kernel<U, K, ABL>>(a, panel_lds_bytes(a.b), (int64_t)a.b->nchunks << 6);
}
template <int U, int K>
void run_paired(const PanelLaunchArgs &a, const PanelPlan &plan) {
  clear_word(a, kArrive);
  if (plan.nslices > 1 && !a.accumulate)  // the slices of a panel add their parts into y
    SPL_HIP(hipMemsetAsync(a.y, 0, (size_t)a.m->nrows_local * sizeof(double), a.s));
  launch_on_image<&spmv_panelw_kernel<U, K>>(a, panel_lds_bytes(a.b), (int64_t)(a.b->nchunks / 2) << 6, plan.nslices);
}
template <int U>
void run_rounds(const PanelLaunchArgs &a, const PanelPlan &plan) {  // the kernel itself puts the rendezvous word back
  const PanelImage *b = a.b;
  launch_panel_kernel<&spmv_panelq_kernel<U>>(a.m->device, a.nb, panel_lds_bytes(b), a.s, a.m->nrows_local, b->npanels, b->P, b->w,
                                              b->nib, b->segc.get(), b->ublk.get(), b->key.get(), b->val.get(), a.x, a.y,
                                              a.accumulate, b->arrive.get(), (int64_t)(b->nchunks / 2) << 6, plan.meet);
}
template <int NL, int D, int GD, int K, int S>
void run_ring(const PanelLaunchArgs &a, const PanelPlan &) {
  clear_word(a, kArrive);
  clear_word(a, kRingError);
  launch_on_image<&spmv_panelr_kernel<NL, D, GD, K, S>>(a, panel_ring_lds_bytes(a.b->P, NL, S), (int64_t)(a.b->nchunks / 2) << 6);
}

// The table of instantiations: a plan runs iff normalise() maps it to one of these.  (nslices is a launch
// argument of the paired kernels, not an instantiation.)
struct PanelKernel {
  PanelForm form;
  int sets, kblocks, ablate, nl, gather, slots;
  void (*run)(const PanelLaunchArgs &, const PanelPlan &);
  const char *where;
};
template <int U, int K, int ABL = 0>
constexpr PanelKernel chunk() {
  return {PanelForm::Chunk, U, K, ABL, 0, 0, 0, &run_chunk<U, K, ABL>, ABL ? "spmv_panel ablation launch" : "spmv_panel launch"};
}
template <int U, int K>
constexpr PanelKernel paired() { return {PanelForm::Paired, U, K, 0, 0, 0, 0, &run_paired<U, K>, "spmv_panelw launch"}; }
template <int U>
constexpr PanelKernel rounds() { return {PanelForm::Rounds, U, 0, 0, 0, 0, 0, &run_rounds<U>, "spmv_panelq launch"}; }
template <int NL, int D, int GD, int K, int S>
constexpr PanelKernel ring() {
  return {PanelForm::Ring, D, K, 0, NL, GD, S, &run_ring<NL, D, GD, K, S>, "spmv_panelr launch"};
}
const PanelKernel kPanelKernels[] = {
    rounds<3>(), rounds<4>(), rounds<5>(), rounds<6>(),
    paired<2, 1>(), paired<3, 1>(), paired<4, 1>(), paired<3, 2>(), paired<4, 2>(), paired<5, 2>(), paired<6, 2>(),
    chunk<4, 1>(), chunk<6, 1>(), chunk<8, 1>(), chunk<10, 1>(), chunk<12, 1>(),
    chunk<4, 2>(), chunk<6, 2>(), chunk<8, 2>(), chunk<10, 2>(), chunk<12, 2>(),
    // timing-only (wrong results): the two-stage kernel, 12 chunks, 2 blocks per phase
    chunk<12, 2, 1>(), chunk<12, 2, 2>(), chunk<12, 2, 3>(), chunk<12, 2, 4>(), chunk<12, 2, 5>(), chunk<12, 2, 6>(),
    chunk<12, 2, 7>(),
    // ring (loaders, loader depth, gatherer depth, blocks per phase, slots): only shapes that compile without
    // scratch — a spilled register with a gather still in flight would be stale
    ring<4, 4, 4, 2, 1>(), ring<4, 6, 4, 2, 1>(), ring<4, 8, 4, 2, 1>(), ring<4, 6, 3, 2, 1>(), ring<4, 6, 4, 1, 1>(),
    ring<4, 6, 4, 2, 3>(), ring<4, 4, 3, 2, 1>(), ring<4, 5, 4, 2, 1>(), ring<2, 8, 2, 2, 1>(), ring<8, 3, 4, 2, 1>(),
    ring<8, 4, 4, 2, 1>(), ring<4, 6, 4, 3, 1>(), ring<4, 6, 4, 4, 1>(), ring<4, 6, 4, 3, 3>(), ring<4, 6, 4, 4, 3>(),
    ring<4, 4, 4, 2, 3>(), ring<4, 6, 3, 2, 3>(), ring<4, 6, 4, 1, 3>(), ring<4, 4, 4, 4, 1>(), ring<4, 4, 4, 3, 1>(),
    ring<8, 4, 4, 4, 1>(), ring<8, 4, 4, 2, 2>(), ring<4, 4, 4, 8, 1>(), ring<4, 6, 4, 8, 1>()};

// A request between the instantiated register counts is served by a fixed neighbour, and fields the form does
// not use are dropped; rounds and ring requests are left alone (no entry in the table: the launch refuses).
PanelPlan normalise(PanelPlan p) {
  const auto one_of = [](int v, std::initializer_list<int> ok) { for (int o : ok) if (v == o) return true; return false; };
  switch (p.form) {
    case PanelForm::Chunk:
      p.kblocks = p.kblocks == 1 ? 1 : 2;
      if (!one_of(p.sets, {4, 6, 8, 10})) p.sets = 12;
      if (p.ablate) { p.sets = 12; p.kblocks = 2; }
      break;
    case PanelForm::Paired:
      p.kblocks = p.kblocks == 1 ? 1 : 2;
      if (p.kblocks == 1 && !one_of(p.sets, {2, 4})) p.sets = 3;
      if (p.kblocks == 2 && !one_of(p.sets, {3, 4, 5})) p.sets = 6;
      break;
    case PanelForm::Rounds: p.kblocks = 0; break;
    case PanelForm::Ring: break;
  }
  if (p.form != PanelForm::Chunk) p.ablate = 0;
  if (p.form != PanelForm::Paired) p.nslices = 1;
  if (p.form != PanelForm::Ring) p.nl = p.gather = p.slots = 0;
  if (p.form != PanelForm::Rounds) p.meet = 1;
  return p;
}

const PanelKernel *find_panel_kernel(const PanelPlan &p) {  // p normalised
  for (const PanelKernel &k : kPanelKernels)
    if (k.form == p.form && k.sets == p.sets && k.kblocks == p.kblocks && k.ablate == p.ablate && k.nl == p.nl &&
        k.gather == p.gather && k.slots == p.slots)
      return &k;
  return nullptr;
}

}  // namespace

int panel_ring_errors(const Matrix *m, hipStream_t s) {
  const PanelImage *b = m->panel;
  if (!b || !b->arrive.get()) return 0;
  unsigned e = 0;
  SPL_HIP(hipMemcpyAsync(&e, b->arrive.get() + kRingError, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  return (int)e;
}

int launch_spmv_panel(const Matrix *m, const PanelPlan &requested, const double *d_x, double *d_y, int accumulate,
                      hipStream_t s) {
  const PanelImage *b = m->panel;
  if (!b) return SPL_ERROR_internal;
  if (b->npanels == 0) return SPL_OK;
  if (m->nnz == 0) {
    if (!accumulate) SPL_HIP(hipMemsetAsync(d_y, 0, (size_t)m->nrows_local * sizeof(double), s));
    return SPL_OK;
  }
  if (panel_lds_bytes(b) > kPanelLdsLimit) return SPL_ERROR_argument_missing;
  const PanelPlan plan = normalise(requested);
  // every form but the chunk form reads the paired storage, the rounds form its unit table too
  if ((plan.form != PanelForm::Chunk) != (b->pair != 0)) return SPL_ERROR_internal;
  if (plan.form == PanelForm::Rounds && !b->ublk.get()) return SPL_ERROR_internal;
  if (plan.form == PanelForm::Ring && panel_ring_lds_bytes(b->P, plan.nl, plan.slots) > kPanelLdsLimit)
    return SPL_ERROR_argument_missing;
  const PanelKernel *k = find_panel_kernel(plan);
  if (!k) return SPL_ERROR_argument_missing;
  const int cus = device_cus(m->device);
  if (cus == 0) { set_last_error_text("hipDeviceGetAttribute(MultiprocessorCount) failed"); return SPL_ERROR_device; }
  int64_t nb = cus;
  const int64_t tasks = b->npanels * plan.nslices;
  if (nb > tasks) nb = tasks;
  k->run(PanelLaunchArgs{m, b, (unsigned)nb, d_x, d_y, accumulate, s}, plan);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_last_error(k->where, e); return SPL_ERROR_device; }
  return SPL_OK;
}

// ---- choosing the plan ------------------------------------------------------------------------------
static int env_int(const char *name, int otherwise) {
  const char *ev = getenv(name);
  return ev ? atoi(ev) : otherwise;
}

int panel_slices_override() { return env_int("SPL_PANEL_SLICES", 0); }  // 0: not set

bool panel_code_valid(int form, int unroll) {  // the codes are 0 ... 11 without 3; rounds of 3 ... 6 register sets
  if (form == SPL_PANEL_FORM_ROUNDS) return unroll == 0 || (unroll >= 3 && unroll <= 6);
  return form >= SPL_PANEL_FORM_DEFAULT && form <= SPL_PANEL_FORM_RING_K8 && form != 3;
}

bool panel_code_takes_slices(int form) {
  return form == SPL_PANEL_FORM_DEFAULT || form == SPL_PANEL_FORM_PAIRED_K1 || form == SPL_PANEL_FORM_PAIRED_K2;
}

// The ABI's numeric codes and the defaults, nowhere else.  sets == 0 (chunk and paired form with unroll 0) is
// left for choose_panel_plan, which sizes it from the image.
PanelPlan panel_plan_from_code(int form, int unroll, int cols_log2, int nslices) {
  // the default: paired, a phase's x window 2 MiB at most (measured on C2, tools/bench_spmv_variants.py:
  // paired 0.90 ms, one chunk per load 0.96 ms)
  if (form == SPL_PANEL_FORM_DEFAULT) form = cols_log2 >= 17 ? SPL_PANEL_FORM_PAIRED_K2 : SPL_PANEL_FORM_PAIRED_K1;
  PanelPlan p;
  p.sets = unroll > 0 ? unroll : 0;
  p.nslices = 1;
  switch (form) {
    case SPL_PANEL_FORM_CHUNK_K1: p.form = PanelForm::Chunk; p.kblocks = 1; break;
    case SPL_PANEL_FORM_CHUNK_K2: p.form = PanelForm::Chunk; p.kblocks = 2; break;
    case SPL_PANEL_FORM_PAIRED_K1: p.form = PanelForm::Paired; p.kblocks = 1; p.nslices = nslices; break;
    case SPL_PANEL_FORM_PAIRED_K2: p.form = PanelForm::Paired; p.kblocks = 2; p.nslices = nslices; break;
    case SPL_PANEL_FORM_ROUNDS:
      p.form = PanelForm::Rounds;
      p.kblocks = 2;
      if (p.sets == 0) p.sets = 5;
      p.meet = env_int("SPL_PANEL_RENDEZVOUS", 1) != 0;  // tests and ablations: an explicit request without the rendezvous
      break;
    default:  // the ring forms, codes 6 ... 10: 1 / 2 / 3 / 4 / 8 index blocks per phase; sets is the depth of a loader
      p.form = PanelForm::Ring;
      p.kblocks = form == SPL_PANEL_FORM_RING_K8 ? 8 : form - SPL_PANEL_FORM_RING_K1 + 1;
      if (p.sets == 0) p.sets = 6;
      p.nl = env_int("SPL_PANEL_RING_NL", 4);
      p.slots = env_int("SPL_PANEL_RING_SLOTS", 1);
      p.gather = env_int("SPL_PANEL_RING_GD", 4);
      break;
  }
  return p;
}

// The register sets per wavefront and the index blocks per phase are worth 5-10 % either way and the best pair sits
// next to the heuristic one (C2: 5 pairs, 2 blocks: 0.90 ms; 6 pairs: 0.97; 4: 0.98; 3 pairs, 1 block: 0.96): time
// the neighbours once (same image; about a hundred launches on a scratch vector) and keep the fastest.  Without column
// slices the rounds form joins with the same register sets +- 1 (C2: 4 pairs 0.82 ms; profiles/panel_rounds_bench.json).
static PanelPlan tune_panel_plan(const Matrix *m, const PanelImage *b, const PanelPlan &heuristic) {
  const int unroll = heuristic.sets, kblocks = heuristic.kblocks;
  const bool verbose = getenv("SPL_PANEL_VERBOSE") != nullptr;
  DBuf<double> tx((size_t)m->ncols), ty((size_t)m->nrows_local);
  SPL_HIP(hipMemsetAsync(tx.get(), 0, (size_t)m->ncols * sizeof(double), nullptr));
  hipEvent_t e0, e1;
  SPL_HIP(hipEventCreate(&e0));
  SPL_HIP(hipEventCreate(&e1));
  std::vector<PanelPlan> cands;
  const auto add = [&](PanelForm form, int k, int u) { PanelPlan c = heuristic; c.form = form; c.kblocks = k; c.sets = u; cands.push_back(c); };
  for (int du = -1; du <= 1; ++du) {
    const int u2 = unroll + du;
    if (kblocks == 2 && u2 >= 3 && u2 <= 6) add(PanelForm::Paired, 2, u2);
    if (kblocks == 1 && u2 >= 2 && u2 <= 4) add(PanelForm::Paired, 1, u2);
  }
  if (kblocks == 2) {
    for (int u1 = (unroll + 1) / 2; u1 <= (unroll + 1) / 2 + 1; ++u1)
      if (u1 >= 2 && u1 <= 4) add(PanelForm::Paired, 1, u1);
  }
  if (heuristic.nslices == 1) {  // the rounds form does not depend on the index blocks: the same register sets +- 1
    const int uq = unroll < 3 ? 3 : unroll > 6 ? 6 : unroll;
    for (int u2 = uq - 1; u2 <= uq + 1; ++u2)
      if (u2 >= 3 && u2 <= 6) {  // with and without the rendezvous between a workgroup's panels
        add(PanelForm::Rounds, kblocks, u2);
        add(PanelForm::Rounds, kblocks, u2);
        cands.back().meet = 0;
      }
  }
  float best_ms = 0.f, heur_ms = 0.f, best_meet_ms = 0.f;
  PanelPlan best = heuristic, best_meet = heuristic;
  for (const PanelPlan &c : cands) {
    const bool q = c.form == PanelForm::Rounds;
    SPL_HIP(hipMemsetAsync(b->arrive.get(), 0, 4 * sizeof(unsigned), nullptr));  // the forms clear it differently
    for (int w = 0; w < 2; ++w) (void)launch_spmv_panel(m, c, tx.get(), ty.get(), 0, nullptr);
    SPL_HIP(hipEventRecord(e0, nullptr));
    for (int r = 0; r < 8; ++r) (void)launch_spmv_panel(m, c, tx.get(), ty.get(), 0, nullptr);
    SPL_HIP(hipEventRecord(e1, nullptr));
    SPL_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    SPL_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (verbose)
      fprintf(stderr, "[panel] candidate %d pairs x %s: %.4f ms\n", c.sets,
              q ? (c.meet ? "rounds" : "rounds, no rendezvous") : c.kblocks == 2 ? "2 blocks" : "1 block", ms / 8.f);
    if (c.kblocks == kblocks && c.sets == unroll && !q) heur_ms = ms;
    if (best_ms == 0.f || ms < best_ms) { best_ms = ms; best = c; }
    if (c.meet && (best_meet_ms == 0.f || ms < best_meet_ms)) { best_meet_ms = ms; best_meet = c; }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  // dropping the rendezvous has to pay by more than 1 % too, against the best candidate that keeps it
  if (!best.meet && best_meet_ms > 0.f && best_ms > 0.99f * best_meet_ms) { best = best_meet; best_ms = best_meet_ms; }
  if (heur_ms > 0.f && best_ms > 0.99f * heur_ms) best = heuristic;  // within noise: keep the heuristic
  if (verbose)
    fprintf(stderr, "[panel] heuristic %d pairs x %d blocks: %.4f ms; chosen %d x %d%s: %.4f ms\n", unroll, kblocks,
            heur_ms / 8.f, best.sets, best.kblocks,
            best.form == PanelForm::Rounds ? (best.meet ? " (rounds)" : " (rounds, no rendezvous)") : "", best_ms / 8.f);
  SPL_HIP(hipMemsetAsync(b->arrive.get(), 0, 4 * sizeof(unsigned), nullptr));
  SPL_HIP(hipStreamSynchronize(nullptr));  // the caller's launches may go to another stream
  return best;
}

PanelPlan choose_panel_plan(const Matrix *m, const PanelImage *b, int form, int unroll, int nslices, bool may_tune) {
  PanelPlan plan = panel_plan_from_code(form, unroll, b->w, nslices);
  if (plan.form == PanelForm::Rounds || plan.form == PanelForm::Ring) return normalise(plan);
  if (unroll == 0) {
    // units (chunks or pairs) per wavefront and phase: the 16 wavefronts share a phase's units evenly.  More loads
    // in flight than the mean needs cost time (the stream then queues in front of the gathers in the CU's L1): the
    // nearest count, and the longer phases take the un-pipelined tail loop (C2: 5 pairs 0.90 ms, 6 pairs 0.97 ms;
    // 69 % of the phases have a tail, profiles/panel_rounds_before.txt — what the rounds form does away with)
    const double per_wave = (double)b->nchunks * plan.kblocks / (double)(b->npanels * b->nib > 0 ? b->npanels * b->nib : 1) / 16.0;
    if (plan.form == PanelForm::Paired) {
      const int pairs = (int)(per_wave / 2.0 + 0.5);
      plan.sets = pairs < 2 ? 2 : pairs > 6 ? 6 : pairs;
    } else {
      const int want = (int)(per_wave + 0.5);
      plan.sets = want <= 4 ? 4 : want <= 6 ? 6 : want <= 8 ? 8 : want <= 10 ? 10 : 12;
    }
  }
  const char *forced = getenv("SPL_PANEL_UNROLL"), *tune = getenv("SPL_PANEL_TUNE");
  if (forced) plan.sets = atoi(forced);
  // only the all-default request on a large matrix is tuned; SPL_PANEL_TUNE=0 keeps the heuristic
  if (may_tune && form == SPL_PANEL_FORM_DEFAULT && unroll == 0 && m->nnz > (int64_t)1 << 22 && !forced &&
      !(tune && tune[0] == '0'))
    plan = tune_panel_plan(m, b, plan);
  const char *ok = getenv("SPL_ALLOW_ABLATION"), *ab = getenv("SPL_PANEL_ABLATE");
  if (ok && ok[0] == '1' && ab && plan.form == PanelForm::Chunk) plan.ablate = atoi(ab) & 7;
  return normalise(plan);  // the plan the image records is the one that runs
}

}  // namespace spl

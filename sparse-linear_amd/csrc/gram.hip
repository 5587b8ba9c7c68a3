// gram.hip — a block of inner products in one pass (spl_vector_gram_dev): G[i][j] = <V[:, i], W[:, j]>, Double and
// packed Complex Double.
//
// The arithmetic is the fold of krylov_fold.hpp, so every entry is spl_vector_dot_dev's bit for bit: chunks of 4096,
// lane t of 256 adds its 16 products in ascending order from +0.0, the halving tree, the partials folded by the same
// fold.  The fold fixes which lane owns which row, so lanes cannot share entries; the reuse is a REGISTER TILE.  A
// workgroup takes (chunk, tile of TW columns of W): the lane keeps its 16 entries of each of the TW columns in
// registers (as dots_kernel keeps w) and streams the columns of V past them, TW sums per column of V.  A column of V
// is then read once per tile of W instead of once per column of W.  lane_tree runs on B columns of V at a time, that
// is B * TW * VW planes per round instead of dots_kernel's 4 * VW.
//
// Workgroups are dealt round-robin over the 8 XCDs, so the work items are numbered to keep a chunk on one XCD:
// workgroup b serves XCD b mod 8, and the workgroups of one XCD walk (chunk, tile) with the tile fastest.  Neighbours
// in an XCD then read the same chunk of V at the same time: it comes from HBM once and the other tiles find it in that
// XCD's L2.  Nothing depends on the placement: an item is a function of its number, and a workgroup writes its own
// partials only.  No floating-point atomic, no kernel waits for another workgroup.
//
// The partials of a call are kb * lb * VW planes of chunks_of(n) doubles.  The entry point tiles the call over blocks
// of columns so that one block's partials fit kGramScratch (64 MiB); the smallest block is B x TW columns, which at
// complex width is n / 16 bytes, so the scratch of a call is bounded by max(64 MiB, n / 16 bytes) plus the middle level.
#include "krylov_fold.hpp"

namespace spl {

namespace {

constexpr int kGramBatch = 4;                           // columns of V per lane_tree round
constexpr size_t kGramScratch = (size_t)64 << 20;       // bytes of first-level partials one block of columns may take
constexpr int kXcds = 8;

// What a launch works on: the block V[:, i0 .. i0 + kb) x W[:, j0 .. j0 + lb) of the whole Gram matrix
struct GramBlock {
  int i0, kb, j0, lb;
  int upper;  // only the entries with i0 + i <= j0 + j are wanted
};

// part[((j * kb + i) * VW + p) * stride + c] = plane p of chunk c of <V[:, i0 + i], W[:, j0 + j]>
template <int VW, int TW>
__global__ __launch_bounds__(kLanes) void gram_kernel(int64_t n, GramBlock b, const double *__restrict__ V, int64_t ldv,
                                                      const double *__restrict__ W, int64_t ldw, double *part,
                                                      int64_t stride) {
  constexpr int B = kGramBatch;
  __shared__ double lds[B * TW * VW * kLanes];
  const int t = threadIdx.x;
  const int64_t nchunks = (n + kChunk - 1) / kChunk;
  const int tiles = (b.lb + TW - 1) / TW;
  const int64_t per_xcd = (nchunks + kXcds - 1) / kXcds * tiles;  // items of one XCD
  for (int64_t wg = blockIdx.x; wg / kXcds < per_xcd; wg += gridDim.x) {
    const int64_t q = wg / kXcds;
    const int64_t c = q / tiles * kXcds + wg % kXcds;
    const int j_first = (int)(q % tiles) * TW;
    if (c >= nchunks) continue;  // the same for every lane of the workgroup
    // upper: the columns of V past the tile's last column of W pair with nothing that is wanted; a tile that lies
    // wholly left of the block's rows (a cut call) has none and is left before anything is loaded
    const int last = b.j0 + (j_first + TW - 1 < b.lb ? j_first + TW - 1 : b.lb - 1);
    const int k_end = b.upper ? (last - b.i0 + 1 < b.kb ? last - b.i0 + 1 : b.kb) : b.kb;
    if (k_end <= 0) continue;
    const int64_t base = c * kChunk + t;
    const bool full = n - c * kChunk >= kChunk;
    Val<VW> wv[TW][kSteps];
#pragma unroll
    for (int j = 0; j < TW; ++j) {
      const int col = j_first + j < b.lb ? j_first + j : j_first;  // a column past the block: computed again, never stored
      const double *w = W + (size_t)(b.j0 + col) * (size_t)ldw * VW;
#pragma unroll
      for (int s = 0; s < kSteps; ++s) {
        const int64_t i = base + (int64_t)s * kLanes;
        wv[j][s] = (full || i < n) ? load_val<VW>(w, i) : Val<VW>();
      }
    }
    for (int col0 = 0; col0 < k_end; col0 += B) {
      double acc[B * TW * VW];
#pragma unroll
      for (int v = 0; v < B * TW * VW; ++v) acc[v] = 0.0;
#pragma unroll
      for (int i = 0; i < B; ++i) {
        if (col0 + i < k_end) {
          const double *col = V + (size_t)(b.i0 + col0 + i) * (size_t)ldv * VW;
#pragma unroll
          for (int s = 0; s < kSteps; ++s) {
            const int64_t r = base + (int64_t)s * kLanes;
            if (full || r < n) {
              const Val<VW> v = conj_of(load_val<VW>(col, r));
#pragma unroll
              for (int j = 0; j < TW; ++j) accumulate(acc + (i * TW + j) * VW, mul(v, wv[j][s]));
            }
          }
        }
      }
      lane_tree<B * TW * VW>(acc, lds);
      if (t == 0) {
#pragma unroll
        for (int i = 0; i < B; ++i)
#pragma unroll
          for (int j = 0; j < TW; ++j)
            if (col0 + i < k_end && j_first + j < b.lb)
#pragma unroll
              for (int p = 0; p < VW; ++p)
                part[(((int64_t)(j_first + j) * b.kb + (col0 + i)) * VW + p) * stride + c] = acc[(i * TW + j) * VW + p];
      }
    }
  }
}

// A middle level (n > 4096^2 only): fold_kernel of krylov_fold.hpp per plane, with the planes of the pairs that `upper`
// leaves out skipped: nothing of them is ever stored, and those behind a tile's last column were never written
template <int VW>
__global__ __launch_bounds__(kLanes) void gram_fold_kernel(GramBlock b, int64_t count, const double *in, int64_t in_stride,
                                                           double *out, int64_t out_stride) {
  const int pair = blockIdx.y / VW, i = pair % b.kb, j = pair / b.kb;
  if (b.upper && b.i0 + i > b.j0 + j) return;  // the whole workgroup
  const double *src = in + (int64_t)blockIdx.y * in_stride;
  chunk_partials<1>(count, out + (int64_t)blockIdx.y * out_stride, 0,
                    [&](int64_t x, double *acc) { acc[0] = acc[0] + src[x]; });
}

// middle_levels of krylov_fold.hpp on gram_fold_kernel: the same levels, the same two parts of the scratch
template <int VW>
Partials gram_middle_levels(const GramBlock &b, int64_t n, double *scratch, hipStream_t s) {
  const int planes = b.kb * b.lb * VW;
  int64_t count = chunks_of(n);
  const int64_t first_stride = count ? count : 1;
  double *cur = scratch, *other = scratch + (size_t)planes * (size_t)first_stride;
  int64_t stride = first_stride;
  int middle = 0;
  while (count > kChunk) {
    ++middle;
    const int64_t next = chunks_of(count);
    hipLaunchKernelGGL((gram_fold_kernel<VW>), dim3(chunk_grid(count), planes), dim3(kLanes), 0, s, b, count,
                       (const double *)cur, stride, other, next);
    std::swap(cur, other);
    stride = next;
    count = next;
  }
  return Partials{cur, stride, (int)count, middle};
}

// The last level: workgroup (i, j) folds the `count` <= 4096 partials of its pair's planes and writes the entry of G
template <int VW>
__global__ __launch_bounds__(kLanes) void gram_last_kernel(GramBlock b, const double *part, int64_t stride, int count,
                                                           double *G, int64_t ldg) {
  const int i = blockIdx.x, j = blockIdx.y, t = threadIdx.x;
  if (b.upper && b.i0 + i > b.j0 + j) return;  // the whole workgroup
  __shared__ double lds[VW * kLanes];
  const double *src = part + ((int64_t)j * b.kb + i) * VW * stride;
  double f[VW];
#pragma unroll
  for (int p = 0; p < VW; ++p) {
    f[p] = 0.0;
    for (int x = t; x < count; x += kLanes) f[p] = f[p] + src[p * stride + x];
  }
  lane_tree<VW>(f, lds);
  if (t == 0) store_val(G + (size_t)(b.j0 + j) * (size_t)ldg * VW, b.i0 + i, from_planes<VW>(f, 0));
}

// W columns of a register tile: the knob (1, 2 or 4, for measurement), else 4 real and 2 complex
int gram_tile(int vw) {
  const char *e = getenv("SPL_GRAM_TILE");
  const long v = e ? atol(e) : 0;
  return v == 1 || v == 2 || v == 4 ? (int)v : vw == 1 ? 4 : 2;
}

// bytes of partials a block of columns may take: the knob (SPL_GRAM_SCRATCH, for tests of the blocked path), else 64 MiB
size_t gram_scratch() {
  const char *e = getenv("SPL_GRAM_SCRATCH");
  const long long v = e ? atoll(e) : 0;
  return v >= 1 ? (size_t)v : kGramScratch;
}

// the kernels it enqueued
template <int VW>
int gram_block_launch(int64_t n, const GramBlock &b, int tw, const double *V, int64_t ldv, const double *W, int64_t ldw,
                       double *G, int64_t ldg, double *scratch, hipStream_t s) {
  const dim3 block(kLanes);
  if (n > 0) {
    const int64_t c1 = chunks_of(n), tiles = (b.lb + tw - 1) / tw, cap = chunk_grid_cap();
    const int64_t items = (c1 + kXcds - 1) / kXcds * kXcds * tiles;
    const dim3 grid((unsigned)(items < cap ? items : cap));
    if (tw == 1) hipLaunchKernelGGL((gram_kernel<VW, 1>), grid, block, 0, s, n, b, V, ldv, W, ldw, scratch, c1);
    else if (tw == 2) hipLaunchKernelGGL((gram_kernel<VW, 2>), grid, block, 0, s, n, b, V, ldv, W, ldw, scratch, c1);
    else hipLaunchKernelGGL((gram_kernel<VW, 4>), grid, block, 0, s, n, b, V, ldv, W, ldw, scratch, c1);
  }
  // with `upper` the planes below the diagonal hold indeterminate pool contents (the blocks of a cut call share the
  // scratch, too): no level reads them, and nothing of them reaches G
  const Partials P = gram_middle_levels<VW>(b, n, scratch, s);
  hipLaunchKernelGGL((gram_last_kernel<VW>), dim3(b.kb, b.lb), block, 0, s, b, P.p, P.stride, P.count, G, ldg);
  return (n > 0 ? 1 : 0) + P.middle + 1;
}

inline int round_up(int v, int to) { return (v + to - 1) / to * to; }

}  // namespace

// G[i][j] = <V[:, i], W[:, j]>, i < k, j < l, of n entries of vw doubles to d_G (column major, ldg entries apart);
// upper: only i <= j.  Enqueues on s; *launches (may be nullptr) grows by the kernels.  Arguments checked by the caller.
int vector_gram(int device, int64_t n, int vw, int k, int l, const double *d_V, int64_t ldv, const double *d_W,
                int64_t ldw, double *d_G, int64_t ldg, int upper, hipStream_t s, int64_t *launches) {
  const int tw = gram_tile(vw);
  // the block of columns whose partials fit kGramScratch: W's side is halved first, then V's
  const int64_t c1 = chunks_of(n), c2 = chunks_of(c1);
  const size_t per_plane = (size_t)((c1 ? c1 : 1) + (c2 ? c2 : 1)) * sizeof(double);
  const size_t planes_most = gram_scratch() / per_plane;
  int kb = k, lb = l;
  while ((size_t)kb * (size_t)lb * (size_t)vw > planes_most && lb > tw) lb = round_up((lb + 1) / 2, tw);
  while ((size_t)kb * (size_t)lb * (size_t)vw > planes_most && kb > kGramBatch) kb = round_up((kb + 1) / 2, kGramBatch);
  DotBlock *block = dot_block_take(device, fold_scratch(n, kb * lb * vw));
  for (int j0 = 0; j0 < l; j0 += lb)
    for (int i0 = 0; i0 < k; i0 += kb) {
      const GramBlock b{i0, k - i0 < kb ? k - i0 : kb, j0, l - j0 < lb ? l - j0 : lb, upper ? 1 : 0};
      if (upper && i0 > j0 + b.lb - 1) continue;  // all of it below the diagonal
      const int enqueued = vw == 1 ? gram_block_launch<1>(n, b, tw, d_V, ldv, d_W, ldw, d_G, ldg, block->buf.get(), s)
                                   : gram_block_launch<2>(n, b, tw, d_V, ldv, d_W, ldw, d_G, ldg, block->buf.get(), s);
      if (launches) *launches += enqueued;
    }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error("vector gram launch", e);
    (void)hipStreamSynchronize(s);
    dot_block_give(block, s, false);
    return SPL_ERROR_device;
  }
  dot_block_give(block, s, true);
  return SPL_OK;
}

}  // namespace spl

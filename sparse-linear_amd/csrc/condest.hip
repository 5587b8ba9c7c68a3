// condest.hip — estimate of ||op(A)^-1||_1 from the factors a Numeric object holds, and the exact ||A||_1 / ||A||_inf
// of the matrix it keeps on the device: the condition number behind spl_umfpack_{di,zi}_condest (umfpack.hip).
//
// The estimator is Higham & Tisseur's block 1-norm power method (SIAM J. Matrix Anal. Appl. 21, 2000, Alg. 2.4; MATLAB's
// condest, SciPy's onenormest) with t columns and itmax = 5.  One driver serves both value widths (1: real, 2: packed
// complex (re, im)); the solves are the caller's: `solve(sys, k, d_X, d_B)` takes k device columns through the factors.
// Every n x t block (X, Y = op(A)^-1 X, S, Z = op(A)^-H S) stays in device memory for the whole call; per iteration the
// host reads O(t) scalars: the column norms of Y, the selected row indices, and the figures of the stopping tests.
//
// Determinism: every reduction is in a fixed order (sums: fixed chunks, fixed trees; maxima and the sign-agreement counts
// are exact), the random +-1 columns come from spl_mix64 keyed by (iteration, column, attempt), and ties between rows go
// to the smaller index — two calls on the same factors give the same bits.
#include <algorithm>
#include <cmath>
#include <vector>

#include "umfpack_impl.hpp"
#include "../../include/spl_synth.h"

namespace spl {

namespace {

constexpr int kThreads = 256;
constexpr int kItMax = 5;
constexpr int kMaxHist = kItMax * kCondestMaxT + kCondestMaxT;

// modulus of entry i of a vector of width w (w = 2: packed (re, im))
__device__ __forceinline__ double entry_abs(const double *v, size_t i, int w) {
  return w == 1 ? fabs(v[i]) : hypot(v[2 * i], v[2 * i + 1]);
}

// workgroup sum in a fixed tree; thread 0 returns it
__device__ double block_sum(double v) {
  __shared__ double part[kThreads / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int k = 0; k < kThreads / 64; ++k) s += part[k];
  __syncthreads();
  return s;
}

// Column 1-norms of Y (n x t, width w), first pass: block (b, c) sums the fixed chunk b of column c
__global__ __launch_bounds__(kThreads) void colnorm_partial_kernel(const double *__restrict__ Y, size_t n, int w,
                                                                   size_t chunk, double *__restrict__ part) {
  const int c = blockIdx.y;
  const size_t i0 = (size_t)blockIdx.x * chunk, i1 = min(n, i0 + chunk);
  const double *col = Y + (size_t)c * n * w;
  double s = 0.0;
  for (size_t i = i0 + threadIdx.x; i < i1; i += kThreads) s += entry_abs(col, i, w);
  s = block_sum(s);
  if (threadIdx.x == 0) part[(size_t)c * gridDim.x + blockIdx.x] = s;
}
// second pass: one workgroup per column adds the partials in order
__global__ __launch_bounds__(kThreads) void colnorm_final_kernel(const double *__restrict__ part, int nparts,
                                                                 double *__restrict__ out) {
  const int c = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nparts; b += kThreads) s += part[(size_t)c * nparts + b];
  s = block_sum(s);
  if (threadIdx.x == 0) out[c] = s;
}

// S = sign(Y): real +-1 (0 -> +1), complex y / |y| (0 -> 1)
__global__ __launch_bounds__(kThreads) void sign_kernel(const double *__restrict__ Y, double *__restrict__ S,
                                                        size_t total, int w) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  if (w == 1) {
    S[i] = Y[i] >= 0.0 ? 1.0 : -1.0;
    return;
  }
  const double re = Y[2 * i], im = Y[2 * i + 1], a = hypot(re, im);
  S[2 * i] = a == 0.0 ? 1.0 : re / a;
  S[2 * i + 1] = a == 0.0 ? 0.0 : im / a;
}

// real columns only: out[j] += #{i : sign(a_i) != sign(B(i, j))}, j < m — |a . b_j| = n for +-1 columns exactly when
// the count is 0 or n (a count, so the atomics are exact)
__global__ __launch_bounds__(kThreads) void disagree_kernel(const double *__restrict__ a, const double *__restrict__ B,
                                                            size_t n, size_t chunk, unsigned long long *__restrict__ out) {
  const int j = blockIdx.y;
  const size_t i0 = (size_t)blockIdx.x * chunk, i1 = min(n, i0 + chunk);
  const double *b = B + (size_t)j * n;
  unsigned long long cnt = 0;
  for (size_t i = i0 + threadIdx.x; i < i1; i += kThreads) cnt += ((a[i] >= 0.0) != (b[i] >= 0.0)) ? 1 : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(out + j, cnt);
}

// a column of width w <- +-scale drawn from spl_mix64 (key: draw_key), imaginary parts 0; key 0: +scale throughout
__global__ __launch_bounds__(kThreads) void random_sign_kernel(double *__restrict__ col, size_t n, int w, uint64_t key,
                                                               double scale) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  col[i * w] = (key && (spl_mix64(key + (uint64_t)i * SPL_GOLDEN) >> 63)) ? -scale : scale;
  if (w == 2) col[2 * i + 1] = 0.0;
}
uint64_t draw_key(int iteration, int column, int attempt) {
  return spl_mix64(((uint64_t)iteration << 40) ^ ((uint64_t)column << 20) ^ (uint64_t)attempt ^ 0xC0DE57ull) | 1ull;
}

// h_i = max_j |Z(i, j)|: the row infinity-norms of Z
__global__ __launch_bounds__(kThreads) void rownorm_kernel(const double *__restrict__ Z, size_t n, int w, int t,
                                                           double *__restrict__ h) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  double m = 0.0;
  for (int j = 0; j < t; ++j) m = fmax(m, entry_abs(Z + (size_t)j * n * w, i, w));
  h[i] = m;
}

// ---- top-t selection: (h, i) ranks before (h', i') when h > h', or h == h' and i < i' --------------------------------
// what the host reads back per iteration
struct CondestSelection {
  int ind[kCondestMaxT];  // the rows selected, in rank order (-1: none)
  int fresh;              // how many of them are outside the history (the first ones)
  int visited_ahead;      // rows of the history that rank before the first row outside it
  double hmax, hbest;     // max_i h_i, and h at the row whose unit vector gave the estimate
};
struct Cand {
  double h;
  int i;  // -1: none
};
__device__ __forceinline__ bool before(const Cand &a, const Cand &b) {
  if (a.i < 0) return false;
  if (b.i < 0) return true;
  return a.h > b.h || (a.h == b.h && a.i < b.i);
}
// the first in that order among the workgroup's candidates; every thread gets it
__device__ Cand block_best(Cand c) {
  __shared__ double sh[kThreads / 64];
  __shared__ int si[kThreads / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    Cand o{__shfl_xor(c.h, off, 64), __shfl_xor(c.i, off, 64)};
    if (before(o, c)) c = o;
  }
  if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6] = c.h; si[threadIdx.x >> 6] = c.i; }
  __syncthreads();
  Cand b{0.0, -1};
  for (int k = 0; k < kThreads / 64; ++k) {
    const Cand o{sh[k], si[k]};
    if (before(o, b)) b = o;
  }
  __syncthreads();
  return b;
}

// first pass: workgroup b ranks the fixed chunk b of h and keeps its first t rows outside the history (skip[i] != 0)
__global__ __launch_bounds__(kThreads) void select_partial_kernel(const double *__restrict__ h,
                                                                  const unsigned char *__restrict__ skip, size_t n,
                                                                  size_t chunk, int t, Cand *__restrict__ out) {
  const size_t i0 = (size_t)blockIdx.x * chunk, i1 = min(n, i0 + chunk);
  Cand prev{0.0, -1};
  for (int r = 0; r < t; ++r) {
    Cand c{0.0, -1};
    for (size_t i = i0 + threadIdx.x; i < i1; i += kThreads) {
      if (skip && skip[i]) continue;
      const Cand e{h[i], (int)i};
      if (prev.i >= 0 && !before(prev, e)) continue;  // ranked already
      if (before(e, c)) c = e;
    }
    c = block_best(c);
    if (threadIdx.x == 0) out[(size_t)blockIdx.x * t + r] = c;
    prev = c;
    if (c.i < 0) {  // the chunk has no more rows: the rest stay empty
      for (int q = r + 1 + (int)threadIdx.x; q < t; q += kThreads) out[(size_t)blockIdx.x * t + q] = Cand{0.0, -1};
      return;
    }
  }
}

// second pass, one workgroup: the first t of all partial candidates, and the figures of the stopping tests
__global__ __launch_bounds__(kThreads) void select_final_kernel(const Cand *__restrict__ cand, int ncand, int t,
                                                                const double *__restrict__ h, const int *__restrict__ hist,
                                                                int nhist, int ind_best, CondestSelection *__restrict__ out) {
  Cand prev{0.0, -1};
  int m = 0;
  Cand first{0.0, -1};
  for (int r = 0; r < t; ++r) {
    Cand c{0.0, -1};
    for (int q = threadIdx.x; q < ncand; q += kThreads) {
      const Cand e = cand[q];
      if (e.i < 0 || (prev.i >= 0 && !before(prev, e))) continue;
      if (before(e, c)) c = e;
    }
    c = block_best(c);
    if (c.i < 0) break;
    if (threadIdx.x == 0) out->ind[r] = c.i;
    if (r == 0) first = c;
    prev = c;
    ++m;
  }
  if (threadIdx.x == 0) {
    // rows of the history that rank before the first row outside it: when there are t of them, the t most promising
    // rows have all been visited
    int c = 0;
    double hmax = first.i >= 0 ? first.h : 0.0;
    for (int k = 0; k < nhist; ++k) {
      const Cand e{h[hist[k]], hist[k]};
      if (before(e, first) || first.i < 0) ++c;
      hmax = fmax(hmax, e.h);
    }
    // fewer than t rows outside the history (n close to the history's size): the best visited ones fill the block
    Cand fprev{0.0, -1};
    for (int r = m; r < t; ++r) {
      Cand b{0.0, -1};
      for (int k = 0; k < nhist; ++k) {
        const Cand e{h[hist[k]], hist[k]};
        if (fprev.i >= 0 && !before(fprev, e)) continue;
        if (before(e, b)) b = e;
      }
      out->ind[r] = b.i;
      fprev = b;
    }
    out->fresh = m;
    out->visited_ahead = c;
    out->hmax = hmax;
    out->hbest = ind_best >= 0 ? h[ind_best] : 0.0;
  }
}

// X = [e_ind(0) ... e_ind(t-1)] (X zeroed before); the rows enter the history
__global__ void unit_scatter_kernel(double *__restrict__ X, size_t n, int w, const CondestSelection *__restrict__ sel,
                                    int t, unsigned char *__restrict__ in_hist) {
  const int j = threadIdx.x;
  if (j >= t) return;
  const int i = sel->ind[j];
  if (i < 0) return;
  X[((size_t)j * n + (size_t)i) * w] = 1.0;
  if (in_hist) in_hist[i] = 1;
}

// ||A||: the largest sum of |a_ij| over a row of the matrix held (width 2: rows 2g of the real embedding of a complex
// matrix, entries 2j, 2j+1 of a row the two real numbers of one complex entry, whatever swap or unit congruence made
// them: their modulus is |a_gj|).  A row's sum is in a fixed order; the maximum of non-negative doubles is exact on their
// bit patterns, so the atomic gives the same bits in any order.
__global__ __launch_bounds__(kThreads) void row_abs_sum_kernel(const int64_t *__restrict__ rp, const int *__restrict__ ci,
                                                               const double *__restrict__ v, size_t nrows, int w,
                                                               unsigned long long *__restrict__ out) {
  const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (g >= nrows) return;
  const size_t r = g * w;
  double s = 0.0;
  for (int64_t p = rp[r]; p < rp[r + 1];) {
    if (w == 2 && (ci[p] & 1) == 0 && p + 1 < rp[r + 1] && ci[p + 1] == ci[p] + 1) {
      s += hypot(v[p], v[p + 1]);
      p += 2;
    } else {
      s += fabs(v[p]);
      p += 1;
    }
  }
  atomicMax(out, (unsigned long long)__double_as_longlong(s));
}

size_t blocks_for(size_t n) { return (n + kThreads - 1) / kThreads; }

}  // namespace

double matrix_abs_norm(const Matrix *rows, int width, hipStream_t s) {
  const size_t nrows = (size_t)rows->nrows_local / (size_t)width;
  DBuf<unsigned long long> d(1);
  SPL_HIP(hipMemsetAsync(d.get(), 0, sizeof(unsigned long long), s));
  if (nrows > 0)
    hipLaunchKernelGGL(row_abs_sum_kernel, dim3((unsigned)blocks_for(nrows)), dim3(kThreads), 0, s, rows->rowptr64.get(),
                       rows->colidx.get(), rows->val.get(), nrows, width, d.get());
  unsigned long long bits = 0;
  SPL_HIP(hipMemcpyAsync(&bits, d.get(), sizeof bits, hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  double norm;
  memcpy(&norm, &bits, sizeof norm);
  return norm;
}

int condest_inverse_norm(int n_, int w, int sys_y, int sys_z, bool p_inf, int t_req, const DeviceSolve &solve,
                         hipStream_t s, CondestResult &res, double *d_witness) {
  const size_t n = (size_t)n_;
  const int t = (int)std::min<size_t>((size_t)t_req, n);
  res = CondestResult{};
  res.t = t;
  const size_t col = n * (size_t)w, blk = col * (size_t)t;
  DBuf<double> X(blk), Y(blk), S(blk), Sold(blk), xbest(col), wbest(col), h(n);
  // chunks of the two-pass reductions depend on n only (the same bits for the same factors)
  const size_t chunk = std::max<size_t>(4096, (n + 255) / 256), nparts = (n + chunk - 1) / chunk;
  DBuf<double> part(nparts * (size_t)t), norms((size_t)t);
  DBuf<Cand> cand(nparts * (size_t)t);
  DBuf<CondestSelection> dsel(1);
  DBuf<unsigned long long> dis(2 * (size_t)t);
  DBuf<unsigned char> in_hist(n);
  DBuf<int> dhist((size_t)kMaxHist);
  SPL_HIP(hipMemsetAsync(in_hist.get(), 0, n, s));
  const dim3 gblk((unsigned)blocks_for(blk / (size_t)w)), gcol((unsigned)blocks_for(n));
  std::vector<double> hn((size_t)t);
  auto column_norms = [&](const double *Yp) {
    hipLaunchKernelGGL(colnorm_partial_kernel, dim3((unsigned)nparts, (unsigned)t), dim3(kThreads), 0, s, Yp, n, w, chunk,
                       part.get());
    hipLaunchKernelGGL(colnorm_final_kernel, dim3((unsigned)t), dim3(kThreads), 0, s, part.get(), (int)nparts, norms.get());
    SPL_HIP(hipMemcpyAsync(hn.data(), norms.get(), (size_t)t * sizeof(double), hipMemcpyDeviceToHost, s));
    SPL_HIP(hipStreamSynchronize(s));
  };
  auto run_solve = [&](int sys, double *out, const double *in) {
    SPL_HIP(hipStreamSynchronize(s));
    ++res.solves;
    return solve(sys, t, out, in);
  };
  // real columns: does column c of M have a column of M (j < c) or of Mold (all t) that it is parallel to?
  auto parallel_count = [&](const double *a, const double *B, int m) {
    if (m == 0) return std::vector<unsigned long long>();
    SPL_HIP(hipMemsetAsync(dis.get(), 0, (size_t)m * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(disagree_kernel, dim3((unsigned)nparts, (unsigned)m), dim3(kThreads), 0, s, a, B, n, chunk, dis.get());
    std::vector<unsigned long long> c((size_t)m);
    SPL_HIP(hipMemcpyAsync(c.data(), dis.get(), (size_t)m * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    SPL_HIP(hipStreamSynchronize(s));
    return c;
  };
  auto is_parallel = [&](unsigned long long d) { return d == 0 || d == n; };
  auto needs_resampling = [&](double *M, int c, const double *Mold) {
    for (unsigned long long d : parallel_count(M + (size_t)c * n, M, c))
      if (is_parallel(d)) return true;
    if (Mold)
      for (unsigned long long d : parallel_count(M + (size_t)c * n, Mold, t))
        if (is_parallel(d)) return true;
    return false;
  };
  // columns parallel to another are replaced by random +-scale; a column that stays parallel after 64 draws (n tiny:
  // there are only 2^(n-1) classes of +-1 columns) is kept, which costs the estimate nothing but an iteration's worth
  auto resample = [&](double *M, const double *Mold, int iteration, double scale) {
    for (int c = 0; c < t; ++c)
      for (int attempt = 1; attempt <= 64 && needs_resampling(M, c, Mold); ++attempt)
        hipLaunchKernelGGL(random_sign_kernel, gcol, dim3(kThreads), 0, s, M + (size_t)c * n, n, 1,
                           draw_key(iteration, c, attempt), scale);
  };
  auto best_of = [&](double &est) {
    int jb = 0;
    for (int j = 1; j < t; ++j)
      if (hn[(size_t)j] > hn[(size_t)jb]) jb = j;
    est = hn[(size_t)jb];
    return jb;
  };
  auto keep_witness = [&](int jb) {
    SPL_HIP(hipMemcpyAsync(xbest.get(), X.get() + (size_t)jb * col, col * sizeof(double), hipMemcpyDeviceToDevice, s));
    SPL_HIP(hipMemcpyAsync(wbest.get(), Y.get() + (size_t)jb * col, col * sizeof(double), hipMemcpyDeviceToDevice, s));
  };
  auto finish = [&](double est) {
    res.norm_inv = est;
    // p = 1: the column of X that reached est; p = inf: the sign vector of the winning column of op(A)^-1 X, i.e. the
    // conjugate sign vector of the winning row of A^-1 (op(A) = A^T / A^H)
    if (d_witness) {
      if (p_inf)
        hipLaunchKernelGGL(sign_kernel, gcol, dim3(kThreads), 0, s, wbest.get(), d_witness, n, w);
      else
        SPL_HIP(hipMemcpyAsync(d_witness, xbest.get(), col * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    SPL_HIP(hipStreamSynchronize(s));
    return UMFPACK_OK;
  };

  if ((size_t)t == n) {  // t = n: X = I gives ||op(A)^-1||_1 exactly in one solve
    SPL_HIP(hipMemsetAsync(X.get(), 0, blk * sizeof(double), s));
    std::vector<CondestSelection> hs(1);
    for (int j = 0; j < t; ++j) hs[0].ind[j] = j;
    SPL_HIP(hipMemcpyAsync(dsel.get(), hs.data(), sizeof(CondestSelection), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(unit_scatter_kernel, dim3(1), dim3(64), 0, s, X.get(), n, w, dsel.get(), t,
                       static_cast<unsigned char *>(nullptr));
    const int st = run_solve(sys_y, Y.get(), X.get());
    if (st < 0) return st;
    column_norms(Y.get());
    double est = 0.0;
    keep_witness(best_of(est));
    res.iterations = 1;
    return finish(est);
  }

  // starting block: ones / n, then +-1 / n columns none of which is parallel to another (real matrices)
  // (complex matrices: real +-1 / n, and no test for parallel columns — the complex algorithm has none)
  for (int c = 0; c < t; ++c)
    hipLaunchKernelGGL(random_sign_kernel, gcol, dim3(kThreads), 0, s, X.get() + (size_t)c * col, n, w,
                       c == 0 ? (uint64_t)0 : draw_key(0, c, 0), 1.0 / (double)n);
  if (w == 1 && t > 1) resample(X.get(), nullptr, 0, 1.0 / (double)n);

  std::vector<int> hist;
  std::vector<int> ind((size_t)t, -1);
  int ind_best = -1;
  double est_old = 0.0, est = 0.0;
  bool have_old = false;  // S_old holds a sign block (k >= 2)
  for (int k = 1;; ++k) {
    res.iterations = k;
    int st = run_solve(sys_y, Y.get(), X.get());
    if (st < 0) return st;
    column_norms(Y.get());
    const int jb = best_of(est);
    // (1) no gain: the previous estimate (and its witness) stands
    if (k >= 2 && !(est > est_old)) {
      est = est_old;
      break;
    }
    ind_best = k >= 2 ? ind[(size_t)jb] : -1;
    keep_witness(jb);
    est_old = est;
    if (k > kItMax) break;
    std::swap(S.p, Sold.p);
    hipLaunchKernelGGL(sign_kernel, gblk, dim3(kThreads), 0, s, Y.get(), S.get(), blk / (size_t)w, w);
    if (w == 1) {
      // (2) every column of S parallel to a column of S_old: the signs repeat, so will the estimate
      if (have_old) {
        bool all = true;
        for (int c = 0; c < t && all; ++c) {
          bool any = false;
          for (unsigned long long d : parallel_count(S.get() + (size_t)c * n, Sold.get(), t)) any |= is_parallel(d);
          all = any;
        }
        if (all) break;
      }
      if (t > 1) resample(S.get(), have_old ? Sold.get() : nullptr, k, 1.0);
    }
    have_old = true;
    st = run_solve(sys_z, Y.get(), S.get());  // Z overwrites Y (its witness column is kept in wbest)
    if (st < 0) return st;
    hipLaunchKernelGGL(rownorm_kernel, gcol, dim3(kThreads), 0, s, Y.get(), n, w, t, h.get());
    const bool exclude = t > 1;  // t = 1: the best row, visited or not (the paper's replacement is for t > 1)
    hipLaunchKernelGGL(select_partial_kernel, dim3((unsigned)nparts), dim3(kThreads), 0, s, h.get(),
                       exclude ? in_hist.get() : nullptr, n, chunk, t, cand.get());
    hipLaunchKernelGGL(select_final_kernel, dim3(1), dim3(kThreads), 0, s, cand.get(), (int)(nparts * (size_t)t), t,
                       h.get(), dhist.get(), exclude ? (int)hist.size() : 0, ind_best, dsel.get());
    CondestSelection sel;
    SPL_HIP(hipMemcpyAsync(&sel, dsel.get(), sizeof sel, hipMemcpyDeviceToHost, s));
    SPL_HIP(hipStreamSynchronize(s));
    // (4) the best row of Z is the one whose unit vector gave est: no unit vector does better
    if (k >= 2 && sel.hmax == sel.hbest) break;
    // (5) the t most promising rows have all been visited
    if (t > 1 && sel.visited_ahead >= t) break;
    SPL_HIP(hipMemsetAsync(X.get(), 0, blk * sizeof(double), s));
    hipLaunchKernelGGL(unit_scatter_kernel, dim3(1), dim3(64), 0, s, X.get(), n, w, dsel.get(), t,
                       exclude ? in_hist.get() : nullptr);
    for (int j = 0; j < t; ++j) ind[(size_t)j] = sel.ind[j];
    if (exclude) {
      for (int j = 0; j < sel.fresh; ++j) hist.push_back(sel.ind[j]);
      SPL_HIP(hipMemcpyAsync(dhist.get(), hist.data(), hist.size() * sizeof(int), hipMemcpyHostToDevice, s));
    }
  }
  return finish(est);
}

}  // namespace spl

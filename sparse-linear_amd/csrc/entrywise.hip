// entrywise.hip — the entry-wise layer on device-resident handles: `cmap` / `scale` and the Num instance's negate / abs /
// signum (Sparse.hs:110-125), conj, the parts and the magnitude of Data.Complex, diag(r) A diag(c), the filters (stored
// zeros, small entries, bands and triangles) and the abs-sums, abs-maxima and norms.
//
// Maps keep the pattern: the pointers and indices are two device-to-device copies and one flat streaming pass runs over
// the values, 8 / 16 bytes read and written per entry.  Everything that needs the row of an entry (scaling, filters,
// bands, row reductions) runs in the row_groups.hpp frame: a group of G = 1, 2, 4 ... 64 lanes takes one row, the host
// picks G from the mean row length.  The filters are two passes — kept entries counted per row, a scan, a stable
// compacting write whose positions come from a ballot — and a band is one run per row found by bisection, the length
// pass, scan and copy pass of submatrix.hip with a window per row.
//
// Nothing is handed out by atomics and no floating-point atomic exists here.  A row's sum is formed by its group in a
// fixed tree; a column's sum is the row sum of the order-preserving transpose (convert.hip) of the moduli; the Frobenius
// sum is a fixed two-level pass.  The only atomics are maxima of non-negative doubles taken on their bit patterns, which
// are exact and give the same bits in any order, a NaN (whose pattern lies above infinity's) included.
// -ffp-contract=off (Makefile): every product and sum below is rounded once.
#include <math.h>

#include "row_groups.hpp"

namespace spl {

namespace {

constexpr unsigned long long kSignBit = 0x8000000000000000ull;

__device__ inline unsigned long long to_bits(double x) { return (unsigned long long)__double_as_longlong(x); }
__device__ inline double from_bits(unsigned long long b) { return __longlong_as_double((long long)b); }
__device__ inline double flip_sign(double x) { return from_bits(to_bits(x) ^ kSignBit); }
__device__ inline double clear_sign(double x) { return from_bits(to_bits(x) & ~kSignBit); }

// `exponent` of RealFloat: frexp's exponent, and 0 for 0
__device__ inline int ghc_exponent(double x) { return x == 0.0 ? 0 : ilogb(x) + 1; }

// `magnitude` of Data.Complex on finite parts (scaleFloat is ldexp there); inf if a part is infinite, else NaN if one
// is no number: the reference's decodeFloat artefact on those is not reproduced
__device__ inline double ghc_magnitude(double x, double y) {
  if (!isfinite(x) || !isfinite(y)) return (isinf(x) || isinf(y)) ? from_bits(0x7FF0000000000000ull) : from_bits(0x7FF8000000000000ull);
  const int ex = ghc_exponent(x), ey = ghc_exponent(y);
  const int k = ex > ey ? ex : ey;
  const double a = ldexp(x, -k), b = ldexp(y, -k);
  const double aa = a * a, bb = b * b;
  return ldexp(sqrt(aa + bb), k);
}

// |a| of stored entry p: the sign bit cleared, or the magnitude of the packed pair
template <int VW>
__device__ inline double modulus(const double *__restrict__ x, int64_t p) {
  if (VW == 1) return clear_sign(x[p]);
  const double2 z = *reinterpret_cast<const double2 *>(x + 2 * p);
  return ghc_magnitude(z.x, z.y);
}

// (a :+ b) * (c :+ d) of Data.Complex
__device__ inline double2 complex_mul(double a, double b, double c, double d) {
  const double ac = a * c, bd = b * d, ad = a * d, bc = b * c;
  return make_double2(ac - bd, ad + bc);
}

// ---- maps ---------------------------------------------------------------------------------------------------------
template <int VW>
__global__ __launch_bounds__(kRowThreads) void map_kernel(const double *__restrict__ Ax, int64_t n, int op, double sre,
                                                          double sim, double *__restrict__ Cx) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; i < n; i += stride) {
    if (VW == 1) {
      const double x = Ax[i];
      double y = x;  // conj, real
      switch (op) {
        case SPL_MAP_negate: y = flip_sign(x); break;
        case SPL_MAP_abs: y = clear_sign(x); break;
        case SPL_MAP_signum: y = x > 0.0 ? 1.0 : x < 0.0 ? -1.0 : x; break;
        case SPL_MAP_imag: y = 0.0; break;
        case SPL_MAP_scale: y = x * sre; break;
        default: break;
      }
      Cx[i] = y;
    } else {
      const double2 z = *reinterpret_cast<const double2 *>(Ax + 2 * i);
      if (op == SPL_MAP_real) { Cx[i] = z.x; continue; }  // the two that give a real handle
      if (op == SPL_MAP_imag) { Cx[i] = z.y; continue; }
      double2 w = z;
      switch (op) {
        case SPL_MAP_negate: w = make_double2(flip_sign(z.x), flip_sign(z.y)); break;
        case SPL_MAP_conj: w = make_double2(z.x, flip_sign(z.y)); break;
        case SPL_MAP_abs: w = make_double2(ghc_magnitude(z.x, z.y), 0.0); break;
        case SPL_MAP_signum:
          if (z.x == 0.0 && z.y == 0.0) {
            w = make_double2(0.0, 0.0);
          } else {
            const double r = ghc_magnitude(z.x, z.y);
            w = make_double2(z.x / r, z.y / r);
          }
          break;
        case SPL_MAP_scale: w = complex_mul(z.x, z.y, sre, sim); break;
        default: break;
      }
      *reinterpret_cast<double2 *>(Cx + 2 * i) = w;
    }
  }
}

// ---- diag(r) A diag(c) --------------------------------------------------------------------------------------------
// (r[i] * a) * c[j]; a vector that is not given is not multiplied with
template <int G, int VW>
__global__ __launch_bounds__(kRowThreads) void scale_rows_cols_kernel(const int64_t *__restrict__ Ap,
                                                                      const int *__restrict__ Aj,
                                                                      const double *__restrict__ Ax, int64_t nr,
                                                                      const double *__restrict__ rv,
                                                                      const double *__restrict__ cv,
                                                                      double *__restrict__ Cx) {
  constexpr int kGroups = kRowThreads / G;
  const int lane = threadIdx.x % G;
  int64_t r = (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  for (; r < nr; r += stride) {
    const int64_t s = Ap[r], e = Ap[r + 1];
    double rre = 1.0, rim = 0.0;
    if (rv) {
      if (VW == 1) rre = rv[r];
      else { rre = rv[2 * r]; rim = rv[2 * r + 1]; }
    }
    for (int64_t p = s + lane; p < e; p += G) {
      if (VW == 1) {
        double x = Ax[p];
        if (rv) x = rre * x;
        if (cv) x = x * cv[Aj[p]];
        Cx[p] = x;
      } else {
        double2 z = *reinterpret_cast<const double2 *>(Ax + 2 * p);
        if (rv) z = complex_mul(rre, rim, z.x, z.y);
        if (cv) {
          const int64_t j = Aj[p];
          z = complex_mul(z.x, z.y, cv[2 * j], cv[2 * j + 1]);
        }
        *reinterpret_cast<double2 *>(Cx + 2 * p) = z;
      }
    }
  }
}

// ---- filters ------------------------------------------------------------------------------------------------------
// SPL_KEEP_nonzero: an entry goes iff it == 0; SPL_KEEP_abs_above: iff |a| <= tol.  A NaN compares false and stays.
template <int VW>
__device__ inline bool kept(const double *__restrict__ x, int64_t p, int keep, double tol) {
  if (keep == SPL_KEEP_nonzero) {
    if (VW == 1) return !(x[p] == 0.0);
    const double2 z = *reinterpret_cast<const double2 *>(x + 2 * p);
    return !(z.x == 0.0 && z.y == 0.0);
  }
  return !(modulus<VW>(x, p) <= tol);
}

template <int G, int VW>
__global__ __launch_bounds__(kRowThreads) void filter_count_kernel(const int64_t *__restrict__ Ap,
                                                                   const double *__restrict__ Ax, int64_t nr, int keep,
                                                                   double tol, int64_t *__restrict__ cnt) {
  constexpr int kGroups = kRowThreads / G;
  const int lane = threadIdx.x % G;
  int64_t r = (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  for (; r < nr; r += stride) {
    const int64_t s = Ap[r], e = Ap[r + 1];
    int n = 0;
    for (int64_t p = s + lane; p < e; p += G) n += kept<VW>(Ax, p, keep, tol);
    n = group_sum<G>(n);  // every lane of the group is here: r is theirs in common
    if (lane == 0) cnt[r] = n;
  }
}

// The stable compacting write, as select_copy_kernel of submatrix.hip: the group walks the row G entries at a time, in
// every step the lanes that keep their entry are counted by a ballot, a lane's place is the count of kept lanes below
// it.  The steps of a row are the same for all lanes of its group, so the group's bits of the ballot are complete.
template <int G, int VW>
__global__ __launch_bounds__(kRowThreads) void filter_write_kernel(const int64_t *__restrict__ Ap,
                                                                   const int *__restrict__ Aj,
                                                                   const double *__restrict__ Ax, int64_t nr, int keep,
                                                                   double tol, const int64_t *__restrict__ Cp,
                                                                   int *__restrict__ Cj, double *__restrict__ Cx) {
  constexpr int kGroups = kRowThreads / G;
  constexpr unsigned long long kGroupMask = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
  const int lane = threadIdx.x % G;
  const int shift = (threadIdx.x & 63) - lane;  // the group's first lane in its wavefront
  int64_t r = (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  for (; r < nr; r += stride) {
    const int64_t s = Ap[r], e = Ap[r + 1];
    int64_t o = Cp[r];
    for (int64_t base = s; base < e; base += G) {
      const int64_t p = base + lane;
      const bool k = p < e && kept<VW>(Ax, p, keep, tol);
      const unsigned long long bits = (__ballot(k) >> shift) & kGroupMask;
      if (k) {
        const int64_t q = o + __popcll(bits & ((1ull << lane) - 1ull));
        Cj[q] = Aj[p];
        move_value<VW>(Ax, p, Cx, q);
      }
      o += __popcll(bits);
    }
  }
}

// ---- bands --------------------------------------------------------------------------------------------------------
// Row i (global) keeps the columns [i + lo, i + hi] cut to [0, ncols): as [c0, c1), formed without leaving int64
// whatever lo and hi are (0 <= i, ncols < 2^31)
__device__ inline void band_window(int64_t i, int64_t ncols, int64_t lo, int64_t hi, int *c0, int *c1) {
  int64_t a, b;
  if (lo <= -i) a = 0;
  else if (lo >= ncols - i) a = ncols;
  else a = i + lo;
  if (hi < -i) b = 0;
  else if (hi >= ncols - 1 - i) b = ncols;
  else b = i + hi + 1;
  *c0 = (int)a;
  *c1 = (int)(b < a ? a : b);
}

// the length pass of a window (submatrix.hip) with a window per row
template <int G>
__global__ __launch_bounds__(kRowThreads) void band_len_kernel(const int64_t *__restrict__ Ap, const int *__restrict__ Aj,
                                                               int64_t nr, int64_t row0, int64_t ncols, int64_t lo,
                                                               int64_t hi, int *__restrict__ len,
                                                               int64_t *__restrict__ first) {
  constexpr int kGroups = kRowThreads / G;
  const int lane = threadIdx.x % G;
  int64_t r = (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  for (; r < nr; r += stride) {
    int c0, c1;
    band_window(row0 + r, ncols, lo, hi, &c0, &c1);
    const int64_t s = Ap[r];
    int n;
    int64_t p;
    run_in_row<G>(Aj, s, (int)(Ap[r + 1] - s), lane, c0, c1, &n, &p);  // every lane of the group is here
    if (lane == 0) {
      len[r] = n;
      first[r] = p;
    }
  }
}

// ---- reductions ---------------------------------------------------------------------------------------------------
// over the G lanes of a group, every lane of it here; both operations commute bit for bit, so all lanes hold the same
template <int G>
__device__ inline double group_add(double v) {
#pragma unroll
  for (int w = 1; w < G; w <<= 1) v += __shfl_xor(v, w, G);
  return v;
}
template <int G>
__device__ inline double group_max_bits(double v) {  // v >= 0 or a NaN without sign: the order of the bit patterns
#pragma unroll
  for (int w = 1; w < G; w <<= 1) {
    const double o = __shfl_xor(v, w, G);
    if (to_bits(o) > to_bits(v)) v = o;
  }
  return v;
}

// per row the sum or the largest of |a|: lane l of the group takes entries l, l + G, ... in order, the group's tree adds
// the G partial sums.  out: one double per row; top: the largest of them all (bit pattern), for the norms
template <int G, int VW>
__global__ __launch_bounds__(kRowThreads) void row_reduce_kernel(const int64_t *__restrict__ Ap,
                                                                 const double *__restrict__ Ax, int64_t nr, int what,
                                                                 double *__restrict__ out,
                                                                 unsigned long long *__restrict__ top) {
  constexpr int kGroups = kRowThreads / G;
  const int lane = threadIdx.x % G;
  int64_t r = (int64_t)blockIdx.x * kGroups + threadIdx.x / G;
  const int64_t stride = (int64_t)gridDim.x * kGroups;
  for (; r < nr; r += stride) {
    const int64_t s = Ap[r], e = Ap[r + 1];
    double v = 0.0;
    if (what == SPL_REDUCE_abs_sum) {
      for (int64_t p = s + lane; p < e; p += G) v += modulus<VW>(Ax, p);
      v = group_add<G>(v);
    } else {
      for (int64_t p = s + lane; p < e; p += G) {
        const double m = modulus<VW>(Ax, p);
        if (to_bits(m) > to_bits(v)) v = m;
      }
      v = group_max_bits<G>(v);
    }
    if (lane == 0) {
      if (out) out[r] = v;
      if (top) atomicMax(top, to_bits(v));
    }
  }
}

// out[j] = max(out[j], |a|) over the entries of column j, on the bit patterns; out was zeroed
template <int VW>
__global__ __launch_bounds__(kRowThreads) void col_max_kernel(const int *__restrict__ Aj, const double *__restrict__ Ax,
                                                              int64_t n, unsigned long long *__restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; i < n; i += stride) atomicMax(out + Aj[i], to_bits(modulus<VW>(Ax, i)));
}

template <int VW>
__global__ __launch_bounds__(kRowThreads) void moduli_kernel(const double *__restrict__ Ax, int64_t n,
                                                             double *__restrict__ m) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  for (; i < n; i += stride) m[i] = modulus<VW>(Ax, i);
}

// *top = the largest |a| of n entries (VW doubles each), or of n non-negative doubles
template <int VW>
__global__ __launch_bounds__(kRowThreads) void max_bits_kernel(const double *__restrict__ Ax, int64_t n,
                                                               unsigned long long *__restrict__ top) {
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  double v = 0.0;
  for (; i < n; i += stride) {
    const double m = modulus<VW>(Ax, i);
    if (to_bits(m) > to_bits(v)) v = m;
  }
  v = group_max_bits<64>(v);  // the loop is left by all lanes before this
  if ((threadIdx.x & 63) == 0) atomicMax(top, to_bits(v));
}

// sum over the workgroup in a fixed order: the wavefronts' trees, then their four sums one after the other
__device__ inline double block_add(double v, double *wave_sums) {
  v = group_add<64>(v);
  if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kRowThreads / 64; ++w) t += wave_sums[w];
  return t;  // thread 0 holds it
}

// The Frobenius sum, first level: partial[b] = sum over the entries of workgroup b's threads of the squared parts, each
// part scaled by 2^-k first (exact, but for what falls below the subnormals).  Thread t takes entries t, t + T, ... in
// order.  The grid is a function of n alone, so the order of all additions is.
template <int VW>
__global__ __launch_bounds__(kRowThreads) void fro_partial_kernel(const double *__restrict__ Ax, int64_t n, int k,
                                                                  double *__restrict__ partial) {
  __shared__ double wave_sums[kRowThreads / 64];
  int64_t i = (int64_t)blockIdx.x * kRowThreads + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kRowThreads;
  double v = 0.0;
  for (; i < n; i += stride) {
    if (VW == 1) {
      const double a = ldexp(Ax[i], -k);
      v += a * a;
    } else {
      const double2 z = *reinterpret_cast<const double2 *>(Ax + 2 * i);
      const double a = ldexp(z.x, -k), b = ldexp(z.y, -k);
      const double aa = a * a, bb = b * b;
      v += aa + bb;
    }
  }
  const double t = block_add(v, wave_sums);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// second level, one workgroup: *out = sum of partial[0 .. m)
__global__ __launch_bounds__(kRowThreads) void fro_final_kernel(const double *__restrict__ partial, int m,
                                                                double *__restrict__ out) {
  __shared__ double wave_sums[kRowThreads / 64];
  double v = 0.0;
  for (int i = threadIdx.x; i < m; i += kRowThreads) v += partial[i];
  const double t = block_add(v, wave_sums);
  if (threadIdx.x == 0) *out = t;
}

int mean_group(const Matrix *A) { return group_for((double)A->nnz / (double)(A->nrows_local > 0 ? A->nrows_local : 1)); }

void copy_pattern(const Matrix *A, Matrix *C, hipStream_t s) {
  SPL_HIP(hipMemcpyAsync(C->rowptr64.get(), A->rowptr64.get(), ((size_t)A->nrows_local + 1) * sizeof(int64_t),
                         hipMemcpyDeviceToDevice, s));
  if (A->nnz > 0)
    SPL_HIP(hipMemcpyAsync(C->colidx.get(), A->colidx.get(), (size_t)A->nnz * sizeof(int), hipMemcpyDeviceToDevice, s));
}

double read_back_bits(const unsigned long long *d, hipStream_t s) {
  unsigned long long h = 0;
  SPL_HIP(hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  double x;
  memcpy(&x, &h, sizeof(x));
  return x;
}

// d_out[j] = sum of |a| over column j of a whole matrix with nnz < 2^31: the values (their moduli, when complex) go
// through the order-preserving transpose, whose rows are then summed like any rows.  Costs the transpose: 12 bytes per
// entry written and read again, and a synchronisation, because the temporaries are released on return.
void column_sums(const Matrix *A, double *d_out, hipStream_t s) {
  const int64_t nnz = A->nnz, nc = A->ncols;
  DBuf<double> moduli;
  const double *v = A->val.get();
  if (A->vw == 2) {
    moduli.alloc((size_t)nnz);
    hipLaunchKernelGGL((moduli_kernel<2>), dim3(grid_flat(nnz)), dim3(kRowThreads), 0, s, A->val.get(), nnz, moduli.get());
    SPL_HIP(hipGetLastError());
    v = moduli.get();
  }
  DBuf<int64_t> Tp((size_t)nc + 1);
  DBuf<int> Ti((size_t)nnz);
  DBuf<double> Tv((size_t)nnz);
  transpose_compressed(A->rowptr.get(), A->colidx.get(), v, A->nrows_local, nc, nnz, Tp.get(), Ti.get(), Tv.get(), s);
  const int g = group_for((double)nnz / (double)nc);
  for_group_and_width(g, 1, [&](auto gc, auto) {
    hipLaunchKernelGGL((row_reduce_kernel<decltype(gc)::value, 1>), dim3(grid_rows(nc, gc)), dim3(kRowThreads), 0, s,
                       Tp.get(), Tv.get(), nc, (int)SPL_REDUCE_abs_sum, d_out, (unsigned long long *)nullptr);
  });
  SPL_HIP(hipGetLastError());
  SPL_HIP(hipStreamSynchronize(s));
}

}  // namespace

// C = the map `op` over A's values on A's pattern.  C's value kind is the caller's: real for SPL_MAP_real / _imag.
void map_handle(const Matrix *A, int op, double sre, double sim, Matrix *C, hipStream_t s) {
  allocate_result(C, A->nnz);
  copy_pattern(A, C, s);
  if (A->nnz > 0) {
    if (A->vw == 1)
      hipLaunchKernelGGL((map_kernel<1>), dim3(grid_flat(A->nnz)), dim3(kRowThreads), 0, s, A->val.get(), A->nnz, op, sre,
                         sim, C->val.get());
    else
      hipLaunchKernelGGL((map_kernel<2>), dim3(grid_flat(A->nnz)), dim3(kRowThreads), 0, s, A->val.get(), A->nnz, op, sre,
                         sim, C->val.get());
    SPL_HIP(hipGetLastError());
  }
  SPL_HIP(hipStreamSynchronize(s));
}

// C[i,j] = (r[i] * a[i,j]) * c[j]; d_r (nrows_local entries) / d_c (ncols entries) may be nullptr: ones, not multiplied
void scale_rows_cols_handle(const Matrix *A, const double *d_r, const double *d_c, Matrix *C, hipStream_t s) {
  allocate_result(C, A->nnz);
  copy_pattern(A, C, s);
  if (A->nnz > 0) {
    if (!d_r && !d_c) {
      SPL_HIP(hipMemcpyAsync(C->val.get(), A->val.get(), (size_t)A->nnz * (size_t)A->vw * sizeof(double),
                             hipMemcpyDeviceToDevice, s));
    } else {
      for_group_and_width(mean_group(A), A->vw, [&](auto g, auto vw) {
        hipLaunchKernelGGL((scale_rows_cols_kernel<decltype(g)::value, decltype(vw)::value>),
                           dim3(grid_rows(A->nrows_local, g)), dim3(kRowThreads), 0, s, A->rowptr64.get(),
                           A->colidx.get(), A->val.get(), A->nrows_local, d_r, d_c, C->val.get());
      });
      SPL_HIP(hipGetLastError());
    }
  }
  SPL_HIP(hipStreamSynchronize(s));
}

// C = the entries of A that `keep` keeps, their order inside every row kept
void filter_handle(const Matrix *A, int keep, double tol, Matrix *C, hipStream_t s) {
  const int64_t nr = A->nrows_local;
  if (nr == 0 || A->nnz == 0) {
    empty_result(C, s);
    SPL_HIP(hipStreamSynchronize(s));
    return;
  }
  DBuf<int64_t> cnt((size_t)nr);
  C->rowptr64.alloc((size_t)nr + 1);
  const int g = mean_group(A);
  for_group_and_width(g, A->vw, [&](auto gc, auto vw) {
    hipLaunchKernelGGL((filter_count_kernel<decltype(gc)::value, decltype(vw)::value>), dim3(grid_rows(nr, gc)),
                       dim3(kRowThreads), 0, s, A->rowptr64.get(), A->val.get(), nr, keep, tol, cnt.get());
  });
  SPL_HIP(hipGetLastError());
  exclusive_scan_i64(cnt.get(), C->rowptr64.get(), nr, s);
  allocate_entries(C, s);
  if (C->nnz > 0) {
    for_group_and_width(g, A->vw, [&](auto gc, auto vw) {
      hipLaunchKernelGGL((filter_write_kernel<decltype(gc)::value, decltype(vw)::value>), dim3(grid_rows(nr, gc)),
                         dim3(kRowThreads), 0, s, A->rowptr64.get(), A->colidx.get(), A->val.get(), nr, keep, tol,
                         C->rowptr64.get(), C->colidx.get(), C->val.get());
    });
    SPL_HIP(hipGetLastError());
  }
  SPL_HIP(hipStreamSynchronize(s));  // `cnt` is released on return
}

// C = the entries of A with lo <= j - (row0 + i) <= hi; lo > hi: `zeros` of the operand's shape
void band_handle(const Matrix *A, int64_t lo, int64_t hi, Matrix *C, hipStream_t s) {
  const int64_t nr = A->nrows_local;
  if (lo > hi || nr == 0 || A->ncols == 0 || A->nnz == 0) {
    empty_result(C, s);
    SPL_HIP(hipStreamSynchronize(s));
    return;
  }
  DBuf<int> len((size_t)nr);
  DBuf<int64_t> first((size_t)nr);
  C->rowptr64.alloc((size_t)nr + 1);
  for_group_and_width(mean_group(A), A->vw, [&](auto g, auto) {
    hipLaunchKernelGGL((band_len_kernel<decltype(g)::value>), dim3(grid_rows(nr, g)), dim3(kRowThreads), 0, s,
                       A->rowptr64.get(), A->colidx.get(), nr, A->row0, A->ncols, lo, hi, len.get(), first.get());
  });
  SPL_HIP(hipGetLastError());
  exclusive_scan_i32_to_i64(len.get(), C->rowptr64.get(), nr, s);
  allocate_entries(C, s);
  if (C->nnz > 0) {
    const int g2 = group_for((double)C->nnz / (double)nr);
    for_group_and_width(g2, A->vw, [&](auto g, auto vw) {
      hipLaunchKernelGGL((run_copy_kernel<decltype(g)::value, decltype(vw)::value>), dim3(grid_rows(nr, g)),
                         dim3(kRowThreads), 0, s, A->colidx.get(), A->val.get(), first.get(), nr, 0, C->rowptr64.get(),
                         C->colidx.get(), C->val.get());
    });
    SPL_HIP(hipGetLastError());
  }
  SPL_HIP(hipStreamSynchronize(s));  // `len` and `first` are released on return
}

// d_out[i] over the rows (axis 1) or d_out[j] over the columns (axis 0, whole matrices): sum or largest of |a|
void reduce_handle(const Matrix *A, int what, int axis, double *d_out, hipStream_t s) {
  if (axis == 1) {
    if (A->nrows_local == 0) return;
    for_group_and_width(mean_group(A), A->vw, [&](auto g, auto vw) {
      hipLaunchKernelGGL((row_reduce_kernel<decltype(g)::value, decltype(vw)::value>),
                         dim3(grid_rows(A->nrows_local, g)), dim3(kRowThreads), 0, s, A->rowptr64.get(), A->val.get(),
                         A->nrows_local, what, d_out, (unsigned long long *)nullptr);
    });
    SPL_HIP(hipGetLastError());
    return;
  }
  if (A->ncols == 0) return;
  if (A->nnz == 0 || what == SPL_REDUCE_abs_max) {
    SPL_HIP(hipMemsetAsync(d_out, 0, (size_t)A->ncols * sizeof(double), s));  // +0.0
    if (A->nnz == 0) return;
    unsigned long long *out = reinterpret_cast<unsigned long long *>(d_out);
    if (A->vw == 1)
      hipLaunchKernelGGL((col_max_kernel<1>), dim3(grid_flat(A->nnz)), dim3(kRowThreads), 0, s, A->colidx.get(),
                         A->val.get(), A->nnz, out);
    else
      hipLaunchKernelGGL((col_max_kernel<2>), dim3(grid_flat(A->nnz)), dim3(kRowThreads), 0, s, A->colidx.get(),
                         A->val.get(), A->nnz, out);
    SPL_HIP(hipGetLastError());
    return;
  }
  column_sums(A, d_out, s);
}

// the 1-, infinity-, Frobenius or max norm of a whole matrix; 0 when it has no entry
double norm_handle(const Matrix *A, int which, hipStream_t s) {
  if (A->nnz == 0 || A->nrows_local == 0 || A->ncols == 0) return 0.0;
  DBuf<unsigned long long> top(1);
  SPL_HIP(hipMemsetAsync(top.get(), 0, sizeof(unsigned long long), s));
  auto largest = [&](const double *x, int64_t n, int vw) {
    const unsigned grid = grid_flat(n, 1024);
    if (vw == 1) hipLaunchKernelGGL((max_bits_kernel<1>), dim3(grid), dim3(kRowThreads), 0, s, x, n, top.get());
    else hipLaunchKernelGGL((max_bits_kernel<2>), dim3(grid), dim3(kRowThreads), 0, s, x, n, top.get());
    SPL_HIP(hipGetLastError());
    return read_back_bits(top.get(), s);
  };
  if (which == SPL_NORM_inf) {
    for_group_and_width(mean_group(A), A->vw, [&](auto g, auto vw) {
      hipLaunchKernelGGL((row_reduce_kernel<decltype(g)::value, decltype(vw)::value>),
                         dim3(grid_rows(A->nrows_local, g)), dim3(kRowThreads), 0, s, A->rowptr64.get(), A->val.get(),
                         A->nrows_local, (int)SPL_REDUCE_abs_sum, (double *)nullptr, top.get());
    });
    SPL_HIP(hipGetLastError());
    return read_back_bits(top.get(), s);
  }
  if (which == SPL_NORM_one) {
    DBuf<double> sums((size_t)A->ncols);
    column_sums(A, sums.get(), s);
    return largest(sums.get(), A->ncols, 1);
  }
  const double m = largest(A->val.get(), A->nnz, A->vw);
  if (which == SPL_NORM_max || m == 0.0 || !(m < HUGE_VAL)) return m;  // fro: 0, inf and NaN are their own answer
  // Frobenius: 2^k sqrt(sum (|a| 2^-k)^2), k the exponent of the max norm: the scaled parts are at most 1 and the
  // largest at least 1/2, so the sum neither overflows nor vanishes
  int k = 0;
  (void)frexp(m, &k);
  const unsigned grid = grid_flat(A->nnz, 1024);
  DBuf<double> partial((size_t)grid + 1);
  if (A->vw == 1)
    hipLaunchKernelGGL((fro_partial_kernel<1>), dim3(grid), dim3(kRowThreads), 0, s, A->val.get(), A->nnz, k, partial.get());
  else
    hipLaunchKernelGGL((fro_partial_kernel<2>), dim3(grid), dim3(kRowThreads), 0, s, A->val.get(), A->nnz, k, partial.get());
  hipLaunchKernelGGL(fro_final_kernel, dim3(1), dim3(kRowThreads), 0, s, partial.get(), (int)grid, partial.get() + grid);
  SPL_HIP(hipGetLastError());
  double sum = 0.0;
  SPL_HIP(hipMemcpyAsync(&sum, partial.get() + grid, sizeof(double), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  return ldexp(sqrt(sum), k);
}

}  // namespace spl

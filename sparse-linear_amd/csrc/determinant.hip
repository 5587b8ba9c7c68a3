// determinant.hip — one pass over the pivots of a factorisation: the product of their absolute values as a
// (mantissa, binary exponent) pair that never overflows, and the counts of negative, of zero and of non-finite pivots
// (inf / NaN: factors that cannot be read; they are left out of the product).
// Behind umfpack_di_get_determinant, spl_umfpack_di_log_determinant and spl_umfpack_inertia (umfpack.hip, which
// adds the signs of the permutations and the scalings each path keeps on the host).
//
// Pivot g lives at base[g] of one of two layouts: band storage (the diagonal AB[doff + g ldab]) or the P panels of the
// multifrontal fronts (pivot j of front f at arena[poff[f] + j (ldp[f] + 1)], f = front_of[g], j = g - p0[f]).  The
// diagonal of a dense front is strided, so a pivot costs about one cache line: the pass is bound by that traffic.
// Determinism: every lane takes fixed pivots, the wavefront and workgroup trees are fixed, and a second launch of one
// workgroup combines the per-workgroup partials in a fixed order — two calls on the same factors give the same bits.
// Rounding: each lane multiplies a handful of mantissas, the rest is a tree, so the relative error of the mantissa
// product grows with log2 n, not with n.
#include "common.hpp"

namespace spl {

namespace {

constexpr int kDetThreads = 256;
constexpr int kDetMaxBlocks = 1024;

struct DetPart {
  double m;       // in [0.5, 1)
  int64_t e;      // binary exponent: product = m 2^e
  int64_t neg;    // pivots < 0
  int64_t zero;   // pivots == 0 (not in m, e)
  int64_t bad;    // pivots that are inf or NaN (not in m, e)
};

// m1, m2 in [0.5, 1): the product lies in [0.25, 1) and one doubling (exact) brings it back
__device__ __forceinline__ void mul_norm(double &m, int64_t &e, double m2, int64_t e2) {
  m *= m2;
  e += e2;
  if (m < 0.5) { m *= 2.0; e -= 1; }
}

__device__ __forceinline__ void take_pivot(double d, double &m, int64_t &e, int64_t &neg, int64_t &zero, int64_t &bad) {
  if (d == 0.0) { ++zero; return; }
  if (!isfinite(d)) { ++bad; return; }
  if (d < 0.0) ++neg;
  int ex = 0;
  const double fr = frexp(fabs(d), &ex);
  mul_norm(m, e, fr, ex);
}

// wavefront, then workgroup tree; thread 0 returns the total
__device__ DetPart reduce_workgroup(double m, int64_t e, int64_t neg, int64_t zero, int64_t bad) {
  __shared__ double sm[kDetThreads / 64];
  __shared__ int64_t se[kDetThreads / 64], sn[kDetThreads / 64], sz[kDetThreads / 64], sb[kDetThreads / 64];
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double om = __shfl_xor(m, off, 64);
    const int64_t oe = __shfl_xor(e, off, 64);
    neg += __shfl_xor(neg, off, 64);
    zero += __shfl_xor(zero, off, 64);
    bad += __shfl_xor(bad, off, 64);
    mul_norm(m, e, om, oe);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { sm[wave] = m; se[wave] = e; sn[wave] = neg; sz[wave] = zero; sb[wave] = bad; }
  __syncthreads();
  DetPart r{0.5, 1, 0, 0, 0};  // 0.5 * 2^1 = 1
  if (threadIdx.x == 0) {
    r = DetPart{sm[0], se[0], sn[0], sz[0], sb[0]};
    for (int w = 1; w < kDetThreads / 64; ++w) {
      mul_norm(r.m, r.e, sm[w], se[w]);
      r.neg += sn[w];
      r.zero += sz[w];
      r.bad += sb[w];
    }
  }
  return r;
}

// pivots g = blockIdx.x + gridDim.x (threadIdx.x + blockDim.x q): workgroup b takes a fixed comb of them
template <bool TREE>
__global__ __launch_bounds__(kDetThreads) void det_partial_kernel(int64_t n, const double *__restrict__ base, int64_t stride,
                                                                  const int *__restrict__ front_of,
                                                                  const int *__restrict__ p0, const int *__restrict__ ldp,
                                                                  const int64_t *__restrict__ poff,
                                                                  DetPart *__restrict__ part) {
  double m = 0.5;
  int64_t e = 1, neg = 0, zero = 0, bad = 0;
  for (int64_t g = (int64_t)blockIdx.x * kDetThreads + threadIdx.x; g < n; g += (int64_t)gridDim.x * kDetThreads) {
    double d;
    if (TREE) {
      const int f = front_of[g];
      const int64_t j = g - p0[f];
      d = base[poff[f] + j * ((int64_t)ldp[f] + 1)];
    } else {
      d = base[g * stride];
    }
    take_pivot(d, m, e, neg, zero, bad);
  }
  const DetPart r = reduce_workgroup(m, e, neg, zero, bad);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

// the partials in a fixed order: thread t takes t, t + 256, ... then the same tree
__global__ __launch_bounds__(kDetThreads) void det_combine_kernel(int count, const DetPart *__restrict__ part,
                                                                  DetPart *__restrict__ out) {
  double m = 0.5;
  int64_t e = 1, neg = 0, zero = 0, bad = 0;
  for (int i = threadIdx.x; i < count; i += kDetThreads) {
    const DetPart p = part[i];
    mul_norm(m, e, p.m, p.e);
    neg += p.neg;
    zero += p.zero;
    bad += p.bad;
  }
  const DetPart r = reduce_workgroup(m, e, neg, zero, bad);
  if (threadIdx.x == 0) *out = r;
}

// Parity of the row interchanges of the threshold pivoting inside the 64 x 64 diagonal blocks (Band::piv = 1).  The
// interchanges are kept only inside the stored inverse M = inv(L11) P_b (diag_block_factor_t): column c of inv(L11),
// unit lower triangular, is stored as column prow_c of M, so the first non-zero row of column p of M is the step c in
// which row p was the pivot.  One wavefront per block; odd blocks are counted (integers: the count is exact).
__global__ __launch_bounds__(256) void block_perm_parity_kernel(int nblocks, const double *__restrict__ invs,
                                                                const int64_t *__restrict__ slot, const int *__restrict__ jb,
                                                                int *__restrict__ odd) {
  const int blk = (int)((blockIdx.x * (unsigned)blockDim.x + threadIdx.x) >> 6), p = threadIdx.x & 63;
  if (blk >= nblocks) return;  // (whole wavefronts: blk is uniform in a wavefront)
  const int w = jb[blk];
  const double *M = invs + slot[blk];
  int c = p;
  if (p < w) {
    c = w;  // (no non-zero: the block is broken; counted as a fixed point)
    for (int r = 0; r < w; ++r)
      if (M[r + (int64_t)p * 64] != 0.0) { c = r; break; }
  }
  // inversions: pairs p < q with c(p) > c(q)
  int inv = 0;
  for (int q = 0; q < 64; ++q) {
    const int cq = __shfl(c, q, 64);
    inv += (p < w && q < w && q > p && cq < c) ? 1 : 0;
  }
  const unsigned long long oddl = __ballot(inv & 1);
  if (p == 0 && (__popcll(oddl) & 1)) atomicAdd(odd, 1);
}

DetResult finish(int blocks, DBuf<DetPart> &part, hipStream_t s) {
  DBuf<DetPart> total(1);
  hipLaunchKernelGGL(det_combine_kernel, dim3(1), dim3(kDetThreads), 0, s, blocks, part.get(), total.get());
  DetPart h{};
  SPL_HIP(hipMemcpyAsync(&h, total.get(), sizeof(DetPart), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  SPL_HIP(hipGetLastError());
  return DetResult{h.m, h.e, h.neg, h.zero, h.bad};
}

int grid_for(int64_t n) {
  int64_t b = (n + kDetThreads * 8 - 1) / (kDetThreads * 8);  // about eight pivots per lane
  return (int)std::max<int64_t>(1, std::min<int64_t>(b, kDetMaxBlocks));
}

}  // namespace

DetResult det_pivots_strided(int64_t n, const double *d_diag, int64_t stride, hipStream_t s) {
  const int blocks = grid_for(n);
  DBuf<DetPart> part((size_t)blocks);
  hipLaunchKernelGGL(det_partial_kernel<false>, dim3(blocks), dim3(kDetThreads), 0, s, n, d_diag, stride, nullptr, nullptr,
                     nullptr, nullptr, part.get());
  return finish(blocks, part, s);
}

DetResult det_pivots_tree(int64_t n, const double *d_arena, const int *d_front_of, const int *d_p0, const int *d_ldp,
                          const int64_t *d_poff, hipStream_t s) {
  const int blocks = grid_for(n);
  DBuf<DetPart> part((size_t)blocks);
  hipLaunchKernelGGL(det_partial_kernel<true>, dim3(blocks), dim3(kDetThreads), 0, s, n, d_arena, (int64_t)0, d_front_of,
                     d_p0, d_ldp, d_poff, part.get());
  return finish(blocks, part, s);
}

int block_pivot_parity(const double *d_invs, const std::vector<int64_t> &slot, const std::vector<int> &jb, hipStream_t s) {
  const int nblocks = (int)slot.size();
  if (nblocks == 0) return 0;
  DBuf<int64_t> dslot(slot.size());
  DBuf<int> djb(jb.size()), odd(1);
  SPL_HIP(hipMemcpyAsync(dslot.get(), slot.data(), slot.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
  SPL_HIP(hipMemcpyAsync(djb.get(), jb.data(), jb.size() * sizeof(int), hipMemcpyHostToDevice, s));
  SPL_HIP(hipMemsetAsync(odd.get(), 0, sizeof(int), s));
  hipLaunchKernelGGL(block_perm_parity_kernel, dim3((unsigned)((nblocks + 3) / 4)), dim3(256), 0, s, nblocks, d_invs,
                     dslot.get(), djb.get(), odd.get());
  int h = 0;
  SPL_HIP(hipMemcpyAsync(&h, odd.get(), sizeof(int), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  SPL_HIP(hipGetLastError());
  return h & 1;
}

}  // namespace spl

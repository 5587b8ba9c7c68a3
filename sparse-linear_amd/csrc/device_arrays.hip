// device_arrays.hip — compressed arrays that are already in device memory, in 32- or 64-bit indices, on their way into
// a handle (spl_matrix_create_csr_dev / _create_csc_dev, abi.hip).  Streaming kernels: the work is memory traffic.
//
// A valid input whose slices ascend is read once and written once:
//   pointers   one pass: checked in the source width and written as the handle's 64-bit pointers
//   indices    one pass: range-checked in the source width, narrowed to int32, written, and compared with their
//              predecessor; 16-byte loads and stores, four indices per thread and step
//   order      "every slice ascends" without knowing, in that pass, where slices begin: the pass counts the positions
//              k > 0 with !(idx[k-1] < idx[k]); a second, short kernel counts those of them that are the first entry of
//              a slice (two narrowed indices per slice).  A descent anywhere else is a slice out of order, so the
//              slices ascend iff the two counts agree.
// Nothing is dereferenced through an index or pointer that has not been checked: the index pass only compares, and the
// per-slice kernel runs on pointers that import_pointers has accepted.
#include "common.hpp"

namespace spl {

namespace {

inline unsigned stream_grid(int64_t items) {  // memory-bound: at most 2048 workgroups, the rest by grid stride
  int64_t b = (items + 255) / 256;
  return (unsigned)(b < 1 ? 1 : b > 2048 ? 2048 : b);
}

constexpr unsigned long long kInvalidBit = 1ull << 63;

// word: 0 on entry; on exit bit 63 = invalid, else the low bits hold ptr[n] (>= 0, so bit 63 is free)
template <typename IT>
__global__ __launch_bounds__(256) void import_ptr_kernel(const IT *__restrict__ ptr, int64_t n,
                                                         int64_t *__restrict__ out,
                                                         unsigned long long *__restrict__ word) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  bool bad = false;
  for (; i <= n; i += stride) {
    const int64_t v = (int64_t)ptr[i];
    out[i] = v;
    bad |= v < 0;
    if (i == 0) bad |= v != 0;
    if (i < n) bad |= v > (int64_t)ptr[i + 1];
    else if (v >= 0) atomicOr(word, (unsigned long long)v);
  }
  if (bad) atomicOr(word, kInvalidBit);
}

template <typename IT>
struct Quad;  // four consecutive indices by 16-byte loads
template <>
struct Quad<int> {
  static __device__ inline void load(const int *p, int64_t v[4]) {
    const int4 q = *reinterpret_cast<const int4 *>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  }
};
template <>
struct Quad<int64_t> {
  static __device__ inline void load(const int64_t *p, int64_t v[4]) {
    const longlong2 a = *reinterpret_cast<const longlong2 *>(p), b = *reinterpret_cast<const longlong2 *>(p + 2);
    v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
  }
};

// stat[0] |= 1: an index outside [0, nminor);  stat[1] += positions k > 0 with !(idx[k-1] < idx[k])  (ORDER only).
// WIDE: idx is 16-byte aligned (out always is: it is a DBuf); else the same walk with one index per load.
template <typename IT, bool ORDER, bool WIDE>
__global__ __launch_bounds__(256) void narrow_check_kernel(const IT *__restrict__ idx, int64_t nnz, int64_t nminor,
                                                           int *__restrict__ out,
                                                           unsigned long long *__restrict__ stat) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t nquad = nnz >> 2;
  bool bad = false;
  unsigned long long desc = 0;
  for (int64_t q = tid; q < nquad; q += stride) {
    const int64_t k = q << 2;
    int64_t v[4];
    if (WIDE) {
      Quad<IT>::load(idx + k, v);
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = (int64_t)idx[k + u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) bad |= v[u] < 0 || v[u] >= nminor;
    if (ORDER) {
      if (k > 0) desc += !((int64_t)idx[k - 1] < v[0]);  // the neighbour quad's last index: a line this wavefront holds
      desc += !(v[0] < v[1]);
      desc += !(v[1] < v[2]);
      desc += !(v[2] < v[3]);
    }
    *reinterpret_cast<int4 *>(out + k) = make_int4((int)v[0], (int)v[1], (int)v[2], (int)v[3]);
  }
  for (int64_t k = (nquad << 2) + tid; k < nnz; k += stride) {  // the last nnz % 4 indices
    const int64_t v = (int64_t)idx[k];
    bad |= v < 0 || v >= nminor;
    if (ORDER && k > 0) desc += !((int64_t)idx[k - 1] < v);
    out[k] = (int)v;
  }
  if (bad) atomicOr(&stat[0], 1ull);
  if (ORDER) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) desc += __shfl_xor(desc, d, 64);
    if ((threadIdx.x & 63) == 0 && desc) atomicAdd(&stat[1], desc);
  }
}

// stat[2] += slices whose first entry k = ptr[r] > 0 has !(idx[k-1] < idx[k]): the descents the order allows
__global__ __launch_bounds__(256) void boundary_descents_kernel(const int64_t *__restrict__ ptr, int64_t nmajor,
                                                                const int *__restrict__ idx,
                                                                unsigned long long *__restrict__ stat) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned long long cnt = 0;
  for (; r < nmajor; r += stride) {
    const int64_t s = ptr[r], e = ptr[r + 1];
    if (e > s && s > 0) cnt += !(idx[s - 1] < idx[s]);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&stat[2], cnt);
}

template <typename IT, bool ORDER>
void launch_narrow_check(const IT *d_idx, int64_t nnz, int64_t nminor, int *out, unsigned long long *stat,
                         hipStream_t s) {
  const dim3 grid(stream_grid((nnz + 3) / 4));
  if ((reinterpret_cast<uintptr_t>(d_idx) & 15u) == 0)
    hipLaunchKernelGGL((narrow_check_kernel<IT, ORDER, true>), grid, dim3(256), 0, s, d_idx, nnz, nminor, out, stat);
  else
    hipLaunchKernelGGL((narrow_check_kernel<IT, ORDER, false>), grid, dim3(256), 0, s, d_idx, nnz, nminor, out, stat);
}

}  // namespace

int64_t import_pointers(int index_width, const void *d_ptr, int64_t nmajor, int64_t *out_ptr64, hipStream_t s) {
  DBuf<unsigned long long> word(1);
  SPL_HIP(hipMemsetAsync(word.get(), 0, sizeof(unsigned long long), s));
  const dim3 grid(stream_grid(nmajor + 1));
  if (index_width == 8)
    hipLaunchKernelGGL(import_ptr_kernel<int64_t>, grid, dim3(256), 0, s, static_cast<const int64_t *>(d_ptr), nmajor,
                       out_ptr64, word.get());
  else
    hipLaunchKernelGGL(import_ptr_kernel<int>, grid, dim3(256), 0, s, static_cast<const int *>(d_ptr), nmajor,
                       out_ptr64, word.get());
  unsigned long long h = 0;
  SPL_HIP(hipMemcpyAsync(&h, word.get(), sizeof(h), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  return (h & kInvalidBit) ? -1 : (int64_t)h;
}

int import_indices(int index_width, const void *d_idx, int64_t nnz, int64_t nminor, const int64_t *d_ptr64,
                   int64_t nmajor, int *out_idx, bool *ascending, hipStream_t s) {
  if (ascending) *ascending = true;
  if (nnz <= 0) return SPL_OK;
  DBuf<unsigned long long> stat(3);
  SPL_HIP(hipMemsetAsync(stat.get(), 0, 3 * sizeof(unsigned long long), s));
  if (index_width == 8) {
    const int64_t *p = static_cast<const int64_t *>(d_idx);
    if (ascending) launch_narrow_check<int64_t, true>(p, nnz, nminor, out_idx, stat.get(), s);
    else launch_narrow_check<int64_t, false>(p, nnz, nminor, out_idx, stat.get(), s);
  } else {
    const int *p = static_cast<const int *>(d_idx);
    if (ascending) launch_narrow_check<int, true>(p, nnz, nminor, out_idx, stat.get(), s);
    else launch_narrow_check<int, false>(p, nnz, nminor, out_idx, stat.get(), s);
  }
  if (ascending && nmajor > 0)
    hipLaunchKernelGGL(boundary_descents_kernel, dim3(stream_grid(nmajor)), dim3(256), 0, s, d_ptr64, nmajor, out_idx,
                       stat.get());
  unsigned long long h[3] = {0, 0, 0};
  SPL_HIP(hipMemcpyAsync(h, stat.get(), sizeof(h), hipMemcpyDeviceToHost, s));
  SPL_HIP(hipStreamSynchronize(s));
  if (h[0]) return SPL_ERROR_invalid_matrix;
  if (ascending) *ascending = h[1] == h[2];
  return SPL_OK;
}

bool device_range_holds(const void *d_p, size_t bytes) {
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void *>(d_p)) != hipSuccess) {
    (void)hipGetLastError();  // not an allocation this runtime made: the caller is trusted, as with host arrays
    return true;
  }
  const size_t off = (size_t)(static_cast<const char *>(d_p) - static_cast<const char *>(base));
  return off <= size && bytes <= size - off;
}

}  // namespace spl

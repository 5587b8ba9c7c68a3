// krylov.hip — preconditioned CG and BiCGSTAB on device handles, Double and packed Complex Double, and the fixed-order
// inner product they are built on.
//
// Arithmetic contract (include/sparse_linear_hip.h).  fold(v, len): v is cut into chunks of 4096 consecutive entries;
// in a chunk lane t of 256 starts from +0.0 and adds the entries t, t + 256, ... in ascending order, and the 256 lane
// sums are folded as s[t] += s[t + h] for h = 128, 64 ... 1.  That is one partial per chunk; the partials are folded by
// the same fold until one value is left.  <a,b> = fold of conj(a_i) * b_i (Data.Complex's product of tri_arith.hpp,
// real and imaginary parts folded apart), every real operation separately rounded (-ffp-contract=off).  The order is a
// function of the length alone: a workgroup takes whole chunks, as many as the grid leaves it, and neither the grid nor
// anything else of the launch shows in the bits.  There is no floating-point atomic and no kernel waits for another
// workgroup: a level of the fold is a launch, and the last level is a launch of ONE workgroup that also does the
// scalar step that consumes the value.  CG without a preconditioner has z = r: <r,z> is the <r,r> just folded, and the
// rho step is done in that launch instead of a second inner product.
//
// Scalars never leave the device.  The solver object keeps a status block (iteration counter, done / reason, rho, alpha,
// beta, omega, |r|^2, |b|^2, the threshold); the one-workgroup kernel that completes an inner product computes the
// scalar that follows from it (IEEE division, Data.Complex's scaled quotient) and lane 0 writes it with ordinary
// stores; the next kernel reads it with plain loads.  Convergence, breakdown, a non-finite residual and max_iter are
// decided there, and every vector kernel of this file reads `done` first and returns without touching a vector once it
// is set: whatever the host launches after that is wasted and changes nothing, so x, the iteration count and the
// history do not depend on how often the host looks at the status block.
#include <math.h>

#include <mutex>
#include <utility>

#include "solver_core.hpp"

namespace spl {

namespace {

// the fold itself (chunks of 4096, 256 lanes, the levels) is krylov_fold.hpp, shared with gmres.hip
constexpr int kMaxPlanes = 4;             // two inner products of two components at most in one pass
constexpr int kDefaultCheckEvery = 16;    // iterations between two looks at the status block (check_every == 0)

// The status block, in device memory (and its copy in pinned host memory).  The packed scalars are 16-byte aligned.
struct Status {
  long long it;   // iterations completed
  int done;       // set once; the vector kernels return when they see it
  int reason;     // 0 converged, 1 max_iter, 2 breakdown, 3 non-finite
  double rho[2], alpha[2], beta[2], omega[2];
  double rr, bb;  // |r|^2 of the recurrence, |b|^2
  double thresh;  // max(rtol sqrt(bb), atol)
  double spare;
};

enum Stage {
  kStageOut = 0,   // the value itself to `out` (spl_vector_dot_dev)
  kStageInit,      // <r,r>, <b,b>: threshold, history[0], the checks of iteration 0
  kStageResidual,  // <r,r>: it += 1, history[it], the checks
  kStageCgRho,     // <r,z>: beta = new / rho (not the first time), rho = new
  kStageCgAlpha,   // <p,q>: alpha = rho / <p,q>
  kStageBiRho,     // <rhat,r>: beta = (new / rho) (alpha / omega) (not the first time), rho = new
  kStageBiAlpha,   // <rhat,v>: alpha = rho / <rhat,v>
  kStageBiHalf,    // <s,s>: the early exit at the half step
  kStageBiOmega,   // <t,s>, <t,t>: omega = <t,s> / <t,t>
  // CG without a preconditioner: z IS r, so <r,z> is the <r,r> this stage has just folded (both parts, when complex),
  // and the rho step follows in the same launch when the checks let the solve go on
  kStageInitRho,     // kStageInit, then kStageCgRho for the first time
  kStageResidualRho  // kStageResidual, then kStageCgRho
};

// partials of ND inner products <a_d, b_d>; a and b may be the same array
template <int VW, int ND>
__global__ __launch_bounds__(kLanes) void dot_kernel(const Status *st, int64_t n, const double *a0, const double *b0,
                                                     const double *a1, const double *b1, double *part, int64_t stride) {
  if (st && st->done) return;
  chunk_partials<VW * ND>(n, part, stride, [&](int64_t i, double *acc) {
    accumulate(acc, mul(conj_of(load_val<VW>(a0, i)), load_val<VW>(b0, i)));
    if (ND == 2) accumulate(acc + VW, mul(conj_of(load_val<VW>(a1, i)), load_val<VW>(b1, i)));
  });
}

// The last level, by ONE workgroup: `count` <= 4096 partials of each of `planes` planes to one value each, and the
// scalar step `stage` on them by lane 0.
template <int VW>
__global__ __launch_bounds__(kLanes) void scalar_kernel(Status *st, int stage, int first, const double *part,
                                                        int64_t stride, int count, int planes, double rtol, double atol,
                                                        long long max_iter, double *hist, double *out) {
  if (st && st->done) return;
  __shared__ double lds[kMaxPlanes * kLanes];
  const int t = threadIdx.x;
  double f[kMaxPlanes];
#pragma unroll
  for (int v = 0; v < kMaxPlanes; ++v) {
    f[v] = 0.0;
    if (v < planes)
      for (int i = t; i < count; i += kLanes) f[v] = f[v] + part[v * stride + i];
  }
  lane_tree<kMaxPlanes>(f, lds);
  if (t != 0) return;
  typedef Val<VW> V;
  const V d0 = from_planes<VW>(f, 0);
  if (stage == kStageOut) {
    out[0] = f[0];
    if (VW == 2) out[1] = f[1];
    return;
  }
  int done = 0, reason = 0;
  auto cg_rho = [&](bool first_time) {
    if (is_zero(d0) || !is_finite(d0)) { done = 1; reason = 2; return; }
    if (!first_time) store_val(st->beta, 0, quot(d0, load_val<VW>(st->rho, 0)));
    store_val(st->rho, 0, d0);
  };
  switch (stage) {
    case kStageInit:
    case kStageInitRho: {
      const double rr = f[0], bb = f[VW];  // the real parts
      const double scaled = rtol * sqrt(bb);
      const double thresh = scaled > atol ? scaled : atol;
      st->rr = rr;
      st->bb = bb;
      st->thresh = thresh;
      if (hist) hist[0] = rr;
      if (!isfinite(rr) || !isfinite(bb)) { done = 1; reason = 3; }
      else if (sqrt(rr) <= thresh) { done = 1; reason = 0; }
      else if (max_iter <= 0) { done = 1; reason = 1; }
      if (stage == kStageInitRho && !done) cg_rho(true);
      break;
    }
    case kStageResidual:
    case kStageResidualRho: {
      const double rr = f[0];
      const long long it = st->it + 1;
      st->it = it;
      st->rr = rr;
      if (hist) hist[it] = rr;
      if (!isfinite(rr)) { done = 1; reason = 3; }
      else if (sqrt(rr) <= st->thresh) { done = 1; reason = 0; }
      else if (it >= max_iter) { done = 1; reason = 1; }
      if (stage == kStageResidualRho && !done) cg_rho(false);
      break;
    }
    case kStageCgRho: {
      cg_rho(first != 0);
      break;
    }
    case kStageCgAlpha:
    case kStageBiAlpha: {
      if (is_zero(d0) || !is_finite(d0)) { done = 1; reason = 2; break; }
      store_val(st->alpha, 0, quot(load_val<VW>(st->rho, 0), d0));
      break;
    }
    case kStageBiRho: {
      if (is_zero(d0) || !is_finite(d0)) { done = 1; reason = 2; break; }
      if (!first) {
        const V a = quot(d0, load_val<VW>(st->rho, 0));
        const V b = quot(load_val<VW>(st->alpha, 0), load_val<VW>(st->omega, 0));
        store_val(st->beta, 0, mul(a, b));
      }
      store_val(st->rho, 0, d0);
      break;
    }
    case kStageBiHalf: {
      const double ss = f[0];
      if (!isfinite(ss)) { done = 1; reason = 3; }
      else if (sqrt(ss) <= st->thresh) {
        const long long it = st->it + 1;
        st->it = it;
        st->rr = ss;
        if (hist) hist[it] = ss;
        done = 1;
        reason = 0;
      }
      break;
    }
    case kStageBiOmega: {
      const V tt = from_planes<VW>(f, 1);
      if (is_zero(tt) || !is_finite(tt)) { done = 1; reason = 2; break; }
      const V w = quot(d0, tt);
      if (is_zero(w) || !is_finite(w)) { done = 1; reason = 2; break; }
      store_val(st->omega, 0, w);
      break;
    }
    default: break;
  }
  if (done) {
    st->reason = reason;
    st->done = 1;
  }
}

// ---- the fused vector steps --------------------------------------------------------------------------------------------
// r = b - q (q == nullptr: r = b and x = 0), rhat = r (when asked for); partials of <r,r> and <b,b>
template <int VW>
__global__ __launch_bounds__(kLanes) void init_kernel(int64_t n, const double *__restrict__ b, const double *__restrict__ q,
                                                      double *__restrict__ x, double *__restrict__ r,
                                                      double *__restrict__ rhat, double *part, int64_t stride) {
  chunk_partials<2 * VW>(n, part, stride, [&](int64_t i, double *acc) {
    const Val<VW> bi = load_val<VW>(b, i);
    Val<VW> ri = bi;
    if (q) ri = sub(bi, load_val<VW>(q, i));
    else store_val(x, i, Val<VW>());
    store_val(r, i, ri);
    if (rhat) store_val(rhat, i, ri);
    accumulate(acc, mul(conj_of(ri), ri));
    accumulate(acc + VW, mul(conj_of(bi), bi));
  });
}

// x += alpha p;  r -= alpha q;  partials of <r,r>
template <int VW>
__global__ __launch_bounds__(kLanes) void cg_update_kernel(const Status *st, int64_t n, const double *__restrict__ p,
                                                           const double *__restrict__ q, double *__restrict__ x,
                                                           double *__restrict__ r, double *part, int64_t stride) {
  if (st->done) return;
  const Val<VW> alpha = load_val<VW>(st->alpha, 0);
  chunk_partials<VW>(n, part, stride, [&](int64_t i, double *acc) {
    store_val(x, i, add(load_val<VW>(x, i), mul(alpha, load_val<VW>(p, i))));
    const Val<VW> ri = sub(load_val<VW>(r, i), mul(alpha, load_val<VW>(q, i)));
    store_val(r, i, ri);
    accumulate(acc, mul(conj_of(ri), ri));
  });
}

// p = z + beta p (first: p = z)
template <int VW>
__global__ __launch_bounds__(kLanes) void cg_direction_kernel(const Status *st, int64_t n, int first, const double *z,
                                                              double *p) {
  if (st->done) return;
  const Val<VW> beta = load_val<VW>(st->beta, 0);
  int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kLanes;
  for (; i < n; i += stride) {
    const Val<VW> zi = load_val<VW>(z, i);
    store_val(p, i, first ? zi : add(zi, mul(beta, load_val<VW>(p, i))));
  }
}

// p = r + beta (p - omega v) (first: p = r)
template <int VW>
__global__ __launch_bounds__(kLanes) void bicg_direction_kernel(const Status *st, int64_t n, int first,
                                                                const double *__restrict__ r,
                                                                const double *__restrict__ v, double *__restrict__ p) {
  if (st->done) return;
  const Val<VW> beta = load_val<VW>(st->beta, 0), omega = load_val<VW>(st->omega, 0);
  int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kLanes;
  for (; i < n; i += stride) {
    const Val<VW> ri = load_val<VW>(r, i);
    if (first) {
      store_val(p, i, ri);
    } else {
      const Val<VW> inner = sub(load_val<VW>(p, i), mul(omega, load_val<VW>(v, i)));
      store_val(p, i, add(ri, mul(beta, inner)));
    }
  }
}

// s = r - alpha v;  x += alpha y;  partials of <s,s>
template <int VW>
__global__ __launch_bounds__(kLanes) void bicg_half_kernel(const Status *st, int64_t n, const double *__restrict__ r,
                                                           const double *__restrict__ v, const double *__restrict__ y,
                                                           double *__restrict__ s, double *__restrict__ x, double *part,
                                                           int64_t stride) {
  if (st->done) return;
  const Val<VW> alpha = load_val<VW>(st->alpha, 0);
  chunk_partials<VW>(n, part, stride, [&](int64_t i, double *acc) {
    const Val<VW> si = sub(load_val<VW>(r, i), mul(alpha, load_val<VW>(v, i)));
    store_val(s, i, si);
    store_val(x, i, add(load_val<VW>(x, i), mul(alpha, load_val<VW>(y, i))));
    accumulate(acc, mul(conj_of(si), si));
  });
}

// x += omega z;  r = s - omega t;  partials of <r,r>.  z may be s itself (no preconditioner): no __restrict__ on them
template <int VW>
__global__ __launch_bounds__(kLanes) void bicg_full_kernel(const Status *st, int64_t n, const double *s, const double *z,
                                                           const double *__restrict__ t, double *__restrict__ x,
                                                           double *__restrict__ r, double *part, int64_t stride) {
  if (st->done) return;
  const Val<VW> omega = load_val<VW>(st->omega, 0);
  chunk_partials<VW>(n, part, stride, [&](int64_t i, double *acc) {
    store_val(x, i, add(load_val<VW>(x, i), mul(omega, load_val<VW>(z, i))));
    const Val<VW> ri = sub(load_val<VW>(s, i), mul(omega, load_val<VW>(t, i)));
    store_val(r, i, ri);
    accumulate(acc, mul(conj_of(ri), ri));
  });
}

// Scratch of spl_vector_dot_dev: a block from the device pool PER CALL, so two calls never share partials, from whatever
// threads and on whatever streams they come.  A call takes a block whose previous user has finished on the device (an
// event recorded behind that user's last kernel says so), or a new one; it records its own event behind its last kernel
// and gives the block back.  Blocks are reused across streams, a finished block that is too small is released, and
// at most kDotBlocksKept finished blocks are kept: nothing grows with the number of streams or calls.  The list lives
// as long as the process (nothing is released at exit, when the runtime may be gone).
constexpr size_t kDotBlocksKept = 8;
std::mutex g_dot_mu;
std::vector<DotBlock *> *dot_blocks() {
  static auto *list = new std::vector<DotBlock *>;
  return list;
}

}  // namespace

DotBlock *dot_block_take(int device, size_t doubles) {
  std::lock_guard<std::mutex> hold(g_dot_mu);
  std::vector<DotBlock *> &list = *dot_blocks();
  DotBlock *found = nullptr;
  size_t idle = 0;
  // The list holds the blocks in flight and at most kDotBlocksKept finished ones, of all devices together: a short walk.
  // A block of another device is asked and released with that device current.
  for (size_t i = 0; i < list.size();) {
    DotBlock *b = list[i];
    bool finished = false, release = false;
    if (!b->taken) {
      if (b->device == device) {
        finished = hipEventQuery(b->done) == hipSuccess;
      } else {
        DeviceGuard other(b->device);
        finished = hipEventQuery(b->done) == hipSuccess;
      }
    }
    if (finished && !found && b->device == device && b->buf.n >= doubles) {
      found = b;
    } else if (finished) {
      const bool too_small = b->device == device && b->buf.n < doubles;  // this call is about to make a larger one
      release = too_small || ++idle > kDotBlocksKept;
    }
    if (release) {
      DeviceGuard owner(b->device);  // no-op on the caller's device
      (void)hipEventDestroy(b->done);
      delete b;
      list.erase(list.begin() + (long)i);
      continue;
    }
    ++i;
  }
  if (!found) {
    std::unique_ptr<DotBlock> b(new DotBlock);
    b->device = device;
    b->buf.alloc(doubles);
    SPL_HIP(hipEventCreateWithFlags(&b->done, hipEventDisableTiming));
    list.push_back(b.get());
    found = b.release();
  }
  found->taken = true;
  return found;
}

// the caller's kernels are enqueued on s (enqueued == false: a launch failed and s was synchronised)
void dot_block_give(DotBlock *b, hipStream_t s, bool enqueued) {
  if (enqueued && hipEventRecord(b->done, s) != hipSuccess) (void)hipStreamSynchronize(s);  // then it is finished for sure
  std::lock_guard<std::mutex> hold(g_dot_mu);
  b->taken = false;
}

namespace {

// the `done` flag of a status block in device memory, for the levels of the fold
inline const int *done_flag(const Status *st) { return st ? &st->done : nullptr; }

template <int VW>
void dot_launch(int64_t n, const double *d_a, const double *d_b, double *d_out, double *scratch, hipStream_t s) {
  const int64_t c1 = chunks_of(n);
  if (c1 > 0)
    hipLaunchKernelGGL((dot_kernel<VW, 1>), dim3(chunk_grid(n)), dim3(kLanes), 0, s, (const Status *)nullptr, n, d_a, d_b,
                       d_a, d_b, scratch, c1);
  const Partials P = middle_levels(nullptr, n, VW, scratch, s);
  hipLaunchKernelGGL((scalar_kernel<VW>), dim3(1), dim3(kLanes), 0, s, (Status *)nullptr, (int)kStageOut, 0, P.p, P.stride,
                     P.count, VW, 0.0, 0.0, 0LL, (double *)nullptr, d_out);
}

}  // namespace

// <a,b> of n entries of vw doubles to d_out (vw doubles, device); enqueues on s.  Arguments checked by the caller.
int vector_dot(int device, int64_t n, int vw, const double *d_a, const double *d_b, double *d_out, hipStream_t s) {
  DotBlock *block = dot_block_take(device, fold_scratch(n, vw));
  if (vw == 1) dot_launch<1>(n, d_a, d_b, d_out, block->buf.get(), s);
  else dot_launch<2>(n, d_a, d_b, d_out, block->buf.get(), s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error("vector dot launch", e);
    (void)hipStreamSynchronize(s);
    dot_block_give(block, s, false);
    return SPL_ERROR_device;
  }
  dot_block_give(block, s, true);
  return SPL_OK;
}

// ---- the solver object (the shared part: solver_core.hpp) ---------------------------------------------------------------
struct Krylov : SolverCore {
  int method;
  Preconditioner pre;
  DBuf<double> hist;  // |r|^2 of every iteration, grown with the iterations issued (room_for)
  StatusBlock<Status> status;
  Krylov(const Matrix *A, int m)
      : SolverCore(kKrylovMagic, A, m == SPL_KRYLOV_cg ? 4 : 8, fold_scratch(A->nrows_local, kMaxPlanes)), method(m) {
    bytes += sizeof(Status);
  }
};

// A: whole and square (the caller checked)
int krylov_create(const Matrix *A, int method, Krylov **out) {
  *out = new Krylov(A, method);
  return SPL_OK;
}

void krylov_set_preconditioner(Krylov *K, TriSolver *T1, const double *d_mid, TriSolver *T2) {
  std::lock_guard<std::mutex> hold(K->lock);
  K->pre.set_parts(T1, d_mid, T2);
}

void krylov_set_preconditioner_amg(Krylov *K, Amg *M) {
  std::lock_guard<std::mutex> hold(K->lock);
  K->pre.set_amg(M);
}

namespace {

// One solve's launches; everything is enqueued on s
template <int VW>
struct Run : LinearRun {
  Krylov *K;
  Status *st;

  Run(Krylov *k, hipStream_t stream, double rt, double at, long long mi, bool history)
      : LinearRun(*k, k->pre, k->hist, stream, rt, at, mi, history), K(k), st(k->status.device.get()) {}

  int64_t stride() const { return chunks_of(n); }
  // the preconditioner's diagonal returns on `done`, as every vector kernel of this file does
  int apply(const double *in, double *out) { return LinearRun::apply<VW>(in, out, done_flag(st)); }

  void scalar(int stage, int first, int dots) {
    const Partials P = middle_levels(done_flag(st), n, dots * VW, scratch, s);
    launches += P.middle + 1;
    hipLaunchKernelGGL((scalar_kernel<VW>), dim3(1), dim3(kLanes), 0, s, st, stage, first, P.p, P.stride, P.count,
                       dots * VW, rtol, atol, max_iter, hist.get(), (double *)nullptr);
  }
  void dot(int stage, int first, const double *a, const double *b) {
    hipLaunchKernelGGL((dot_kernel<VW, 1>), dim3(chunked), dim3(kLanes), 0, s, (const Status *)st, n, a, b, a, b, scratch,
                       stride());
    ++launches;
    scalar(stage, first, 1);
  }
  void dot2(int stage, const double *a0, const double *b0, const double *a1, const double *b1) {
    hipLaunchKernelGGL((dot_kernel<VW, 2>), dim3(chunked), dim3(kLanes), 0, s, (const Status *)st, n, a0, b0, a1, b1,
                       scratch, stride());
    ++launches;
    scalar(stage, 0, 2);
  }
  // r = b - A x (use_x0) or r = b, x = 0; the threshold and the checks of iteration 0.  q: room for A x
  int start(const double *b, double *x, int use_x0, double *q, double *r, double *rhat, int stage = kStageInit) {
    SPL_HIP(hipMemsetAsync(st, 0, sizeof(Status), s));
    if (use_x0) {
      const int e = spmv(x, q);
      if (e != SPL_OK) return e;
    }
    hipLaunchKernelGGL((init_kernel<VW>), dim3(chunked), dim3(kLanes), 0, s, n, b, use_x0 ? (const double *)q : nullptr, x,
                       r, rhat, scratch, stride());
    scalar(stage, 0, 2);
    return SPL_OK;
  }
  long long batch_end(long long issued, int every) const { return issued + every < max_iter ? issued + every : max_iter; }
  const Status &look() { return LinearRun::look(K->status); }

  int cg_iteration(double *x, double *r, double *z, double *p, double *q) {
    int e = spmv(p, q);
    if (e != SPL_OK) return e;
    dot(kStageCgAlpha, 0, p, q);
    hipLaunchKernelGGL((cg_update_kernel<VW>), dim3(chunked), dim3(kLanes), 0, s, (const Status *)st, n, p, q, x, r, scratch,
                       stride());
    ++launches;
    if (pre.set()) {
      scalar(kStageResidual, 0, 1);
      if ((e = apply(r, z)) != SPL_OK) return e;
      dot(kStageCgRho, 0, r, z);
    } else {
      scalar(kStageResidualRho, 0, 1);  // z is r: <r,z> is the <r,r> just folded
    }
    hipLaunchKernelGGL((cg_direction_kernel<VW>), dim3(flat), dim3(kLanes), 0, s, (const Status *)st, n, 0, z, p);
    ++launches;
    return launch_status("krylov cg iteration");
  }

  int bicgstab_iteration(int first, double *x, double *r, double *rhat, double *p, double *v, double *y, double *sv,
                         double *z, double *t) {
    dot(kStageBiRho, first, rhat, r);
    hipLaunchKernelGGL((bicg_direction_kernel<VW>), dim3(flat), dim3(kLanes), 0, s, (const Status *)st, n, first, r, v, p);
    ++launches;
    int e;
    if (pre.set() && (e = apply(p, y)) != SPL_OK) return e;
    if ((e = spmv(y, v)) != SPL_OK) return e;
    dot(kStageBiAlpha, 0, rhat, v);
    hipLaunchKernelGGL((bicg_half_kernel<VW>), dim3(chunked), dim3(kLanes), 0, s, (const Status *)st, n, r, v, y, sv, x,
                       scratch, stride());
    ++launches;
    scalar(kStageBiHalf, 0, 1);
    if (pre.set() && (e = apply(sv, z)) != SPL_OK) return e;
    if ((e = spmv(z, t)) != SPL_OK) return e;
    dot2(kStageBiOmega, t, sv, t, t);
    hipLaunchKernelGGL((bicg_full_kernel<VW>), dim3(chunked), dim3(kLanes), 0, s, (const Status *)st, n, sv, z, t, x, r,
                       scratch, stride());
    ++launches;
    scalar(kStageResidual, 0, 1);
    return launch_status("krylov bicgstab iteration");
  }

  int solve(const double *b, double *x, int use_x0, int check_every, Status *last) {
    const int every = check_every > 0 ? check_every : kDefaultCheckEvery;
    const bool pre = this->pre.set();
    int e;
    int64_t per_iteration = 0;
    room_for(hist, batch_end(0, every) + 1, 0, max_iter);
    if (K->method == SPL_KRYLOV_cg) {
      double *r = K->vec(0), *z = pre ? K->vec(1) : r, *p = K->vec(2), *q = K->vec(3);
      if ((e = start(b, x, use_x0, q, r, nullptr, pre ? kStageInit : kStageInitRho)) != SPL_OK) return e;
      if (pre) {
        if ((e = apply(r, z)) != SPL_OK) return e;
        dot(kStageCgRho, 1, r, z);
      }
      hipLaunchKernelGGL((cg_direction_kernel<VW>), dim3(flat), dim3(kLanes), 0, s, (const Status *)st, n, 1, z, p);
      if ((e = launch_status("krylov cg start")) != SPL_OK) return e;
      for (long long issued = 0; issued < max_iter;) {
        if (issued % every == 0) room_for(hist, batch_end(issued, every) + 1, issued + 1, max_iter);
        const int64_t before = launches;
        if ((e = cg_iteration(x, r, z, p, q)) != SPL_OK) return e;
        per_iteration = launches - before;
        ++issued;
        if ((issued % every == 0 || issued == max_iter) && look().done) break;
      }
    } else {
      double *r = K->vec(0), *rhat = K->vec(1), *p = K->vec(2), *v = K->vec(3), *y = pre ? K->vec(4) : p, *sv = K->vec(5),
             *z = pre ? K->vec(6) : sv, *t = K->vec(7);
      if ((e = start(b, x, use_x0, v, r, rhat)) != SPL_OK) return e;
      if ((e = launch_status("krylov bicgstab start")) != SPL_OK) return e;
      for (long long issued = 0; issued < max_iter;) {
        if (issued % every == 0) room_for(hist, batch_end(issued, every) + 1, issued + 1, max_iter);
        const int64_t before = launches;
        if ((e = bicgstab_iteration(issued == 0, x, r, rhat, p, v, y, sv, z, t)) != SPL_OK) return e;
        per_iteration = launches - before;
        ++issued;
        if ((issued % every == 0 || issued == max_iter) && look().done) break;
      }
    }
    *last = look();
    K->last_launches = per_iteration;
    return SPL_OK;
  }
};

template <int VW>
int solve_width(Krylov *K, const double *d_b, double *d_x, int use_x0, double rtol, double atol, int64_t max_iter,
                int check_every, int64_t result[4], double *history, hipStream_t s) {
  Run<VW> run(K, s, rtol, atol, (long long)max_iter, history != nullptr);
  Status last;
  memset(&last, 0, sizeof(last));
  const int e = run.solve(d_b, d_x, use_x0, check_every, &last);
  if (e != SPL_OK) {
    (void)hipStreamSynchronize(s);
    return e;
  }
  result[0] = last.it;
  result[1] = last.done ? last.reason : 1;
  result[2] = run.spmvs;
  result[3] = run.applications;
  if (history) {
    SPL_HIP(hipMemcpyAsync(history, run.hist.get(), ((size_t)last.it + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
    SPL_HIP(hipStreamSynchronize(s));
    for (long long i = 0; i <= last.it; ++i) history[i] = sqrt(history[i]);  // |r|^2 came down: the norm is its root
  }
  K->last_rounds = last.it;
  ++K->solves;
  return SPL_OK;
}

}  // namespace

// arguments checked by the caller; n > 0.  Enqueues on s and synchronises it: the result is read back.
int krylov_solve(Krylov *K, const double *d_b, double *d_x, int use_x0, double rtol, double atol, int64_t max_iter,
                 int check_every, int64_t result[4], double *history, hipStream_t s) {
  std::lock_guard<std::mutex> hold(K->lock);
  if (K->vw == 1) return solve_width<1>(K, d_b, d_x, use_x0, rtol, atol, max_iter, check_every, result, history, s);
  return solve_width<2>(K, d_b, d_x, use_x0, rtol, atol, max_iter, check_every, result, history, s);
}

void krylov_info(Krylov *K, int64_t info[8]) {
  std::lock_guard<std::mutex> hold(K->lock);
  K->fill_info(info, K->method, K->pre.flags());
}

void krylov_delete(Krylov *K) { delete_object(K); }

}  // namespace spl

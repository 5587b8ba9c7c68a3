// solver_core.hpp — what the iterative objects on device handles share on the host: the object (SolverCore: krylov.hip,
// gmres.hip, eigsh.hip, lobpcg.hip), the status block in device and pinned memory, and what one solve's launches have in
// common (RunCore, with the one reduction of a first level's partials to a scalar; LinearRun for the three that solve
// A x = b with a preconditioner and a history: CG, BiCGSTAB, GMRES).  What differs between the solvers (status structs,
// tables, stages, iteration bodies) is in their files.  Included by those four files only.
#pragma once

#include "history_room.hpp"
#include "precond.hpp"

namespace spl {
namespace {

// The object behind a solver handle: A is borrowed, the work vectors and the scratch of the fold are its own
struct SolverCore : ObjectHead {
  const Matrix *A;
  DBuf<double> work;     // nvec vectors
  DBuf<double> scratch;  // partials of the fold
  size_t bytes;          // of device memory; the owner adds its tables and its status block
  std::mutex lock;       // one solve at a time
  int64_t solves = 0, last_launches = 0;
  int64_t last_rounds = 0;  // of the last solve: iterations (CG, BiCGSTAB, GMRES, LOBPCG) or cycles (Lanczos)
  // A: whole and square (the caller checked)
  SolverCore(uint32_t magic, const Matrix *a, size_t nvec, size_t scratch_doubles) : ObjectHead(magic), A(a) {
    device = a->device;
    vw = a->vw;
    n = a->nrows_local;
    work.alloc(nvec * (size_t)n * (size_t)vw);
    scratch.alloc(scratch_doubles);
    bytes = (nvec * (size_t)n * (size_t)vw + scratch_doubles) * sizeof(double);
  }
  double *vec(int i) const { return work.get() + (size_t)i * (size_t)n * (size_t)vw; }

  // The tail of a *_solve, under the lock: run(Width<VW>(), &launches) at the object's value width returns the status
  // and the kernels it launched; an error synchronises s and records nothing.  *rounds is read after the run
  template <int VW>
  struct Width {
    static constexpr int value = VW;
  };
  template <typename Run>
  int solve_and_record(hipStream_t s, const int64_t *rounds, Run &&run) {
    int64_t launches = 0;
    const int e = vw == 1 ? run(Width<1>(), &launches) : run(Width<2>(), &launches);
    if (e != SPL_OK) {
      (void)hipStreamSynchronize(s);
      return e;
    }
    last_rounds = *rounds;
    last_launches = launches;
    ++solves;
    return SPL_OK;
  }
  // The six slots every *_info fills alike, under the lock; `option` (the method, the restart, ncv, the block) and the
  // flag bits above bit 0 are the solver's
  void fill_info(int64_t info[8], int64_t option, int flags) const {
    info[0] = n;
    info[1] = option;
    info[2] = (vw == 2 ? 1 : 0) | flags;
    info[3] = (int64_t)bytes;
    info[4] = solves;
    info[5] = last_rounds;
    info[6] = last_launches;
    info[7] = 0;
  }
};

// A solver's status block in device memory and its copy in pinned host memory, with `host_extra` bytes behind the copy
template <typename StatusT>
struct StatusBlock {
  DBuf<StatusT> device;
  StatusT *pinned = nullptr;
  explicit StatusBlock(size_t host_extra = 0) : device(1) {
    SPL_HIP(hipHostMalloc(reinterpret_cast<void **>(&pinned), sizeof(StatusT) + host_extra, hipHostMallocDefault));
  }
  StatusBlock(const StatusBlock &) = delete;
  StatusBlock &operator=(const StatusBlock &) = delete;
  ~StatusBlock() {
    if (pinned) (void)hipHostFree(pinned);
  }
};

// One solve's launches; everything is enqueued on s
struct RunCore {
  hipStream_t s;
  int64_t n;
  double *scratch;
  unsigned flat, chunked;
  int64_t launches = 0;

  RunCore(const SolverCore &c, hipStream_t stream)
      : s(stream), n(c.n), scratch(c.scratch.get()), flat(grid_flat(c.n, 4096)), chunked(chunk_grid(c.n)) {}

  int launch_status(const char *where) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return SPL_OK;
    set_last_error(where, e);
    (void)hipStreamSynchronize(s);
    return SPL_ERROR_device;
  }
  // the status block as it is once everything enqueued so far is done; `more`: copies to enqueue beside it
  template <typename StatusT, typename More>
  const StatusT &look(const StatusBlock<StatusT> &b, More more) {
    SPL_HIP(hipMemcpyAsync(b.pinned, b.device.get(), sizeof(StatusT), hipMemcpyDeviceToHost, s));
    more();
    SPL_HIP(hipStreamSynchronize(s));
    return *b.pinned;
  }
  template <typename StatusT>
  const StatusT &look(const StatusBlock<StatusT> &b) {
    return look(b, [] {});
  }
  // A first level left its partials of ONE plane in scratch: the middle levels, for a one-workgroup kernel to read the
  // last level (sum_partials) ...
  Partials last_level() {
    const Partials P = middle_levels(nullptr, n, 1, scratch, s);
    launches += P.middle;
    return P;
  }
  // ... or the whole fold to the double *out
  void fold_to(double *out) {
    const Partials P = last_level();
    hipLaunchKernelGGL(fold_kernel, dim3(1, 1), dim3(kLanes), 0, s, (const int *)nullptr, (int64_t)P.count, P.p, P.stride,
                       out, (int64_t)1);
    ++launches;
  }
};

// The history of a solve in device memory, as room_for (history_room.hpp) grows it: before the first launch and right
// after a look, when s is idle
struct HistoryStore {
  DBuf<double> &buf;
  hipStream_t s;
  bool is_wanted;
  bool wanted() const { return is_wanted; }
  double *get() const { return is_wanted ? buf.get() : nullptr; }  // nullptr: the kernels write no history
  long long capacity() const { return (long long)buf.n; }
  void grow(long long want, long long written) {
    DBuf<double> bigger((size_t)want);
    if (written > 0) {
      SPL_HIP(hipMemcpyAsync(bigger.get(), buf.get(), (size_t)written * sizeof(double), hipMemcpyDeviceToDevice, s));
      SPL_HIP(hipStreamSynchronize(s));  // the old block goes back to the pool on the next line
    }
    buf = std::move(bigger);
  }
};

// The launches of a solve of A x = b: the product, the preconditioner and the history
struct LinearRun : RunCore {
  const Matrix *A;
  const Preconditioner &pre;
  HistoryStore hist;
  double rtol, atol;
  long long max_iter;
  int64_t spmvs = 0, applications = 0;

  LinearRun(const SolverCore &c, const Preconditioner &p, DBuf<double> &history_buf, hipStream_t stream, double rt,
            double at, long long mi, bool history)
      : RunCore(c, stream), A(c.A), pre(p), hist{history_buf, stream, history}, rtol(rt), atol(at), max_iter(mi) {}

  int spmv(const double *x, double *y) {
    ++spmvs;
    ++launches;
    return launch_spmv(A, x, y, 0, s);
  }
  // out = M^-1 in; called only when a part is set.  stop: see Preconditioner::apply
  template <int VW>
  int apply(const double *in, double *out, const int *stop) {
    ++applications;
    return pre.apply<VW>(stop, n, in, out, flat, s, &launches);
  }
};

}  // namespace
}  // namespace spl

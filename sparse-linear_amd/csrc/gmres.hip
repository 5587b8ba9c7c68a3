// gmres.hip — right-preconditioned restarted GMRES on device handles, Double and packed Complex Double, and the fused
// multi-vector inner product its orthogonalisation is built on (spl_vector_dots_dev).
//
// The arithmetic is the fold of krylov_fold.hpp and the sequence of include/sparse_linear_hip.h ("restarted GMRES").
// The orthogonalisation is classical Gram-Schmidt done twice: the j + 1 coefficients of a pass come from ONE kernel that
// loads a chunk of w once and streams the basis past it (dots_kernel), one kernel applies them (update_kernel), and both
// are repeated; the second update leaves the partials of <w,w>.  Every value is what j + 1 separate inner products and
// j + 1 separate updates would give, bit for bit.
//
// Scalars never leave the device.  The Hessenberg column, the rotations, g, the decisions and the history are the work
// of ONE workgroup behind the folds (step_kernel: a lane does the serial part, at most `restart` rotations); the
// back-substitution at a close is one workgroup too.  Both write the status block and the tables with ordinary stores.
// The host cannot know how long a cycle is: it issues all `restart` steps and the close, and every kernel of a step
// reads `skip` (cycle closed, or done) first and returns without touching a vector when it is set.  No kernel waits for
// another workgroup, there is no floating-point atomic and no captured graph.
#include "krylov_basis.hpp"
#include "solver_core.hpp"

namespace spl {

namespace {

// The status block, in device memory (and its copy in pinned host memory)
struct GStatus {
  long long it;      // iterations completed
  long long cycles;  // cycles started
  int done;          // set once, at a cycle start; everything returns when it is set
  int reason;        // 0 converged, 1 max_iter, 2 breakdown, 3 non-finite
  int skip;          // the cycle is closed, or done: the kernels of a step return
  int pending;       // reason + 1 of a breakdown inside the cycle; the solve ends behind the close
  int k;             // columns of the closed cycle
  int spare;
  double rr, bb;     // |r|^2 at the last cycle start, |b|^2
  double thresh;     // max(rtol sqrt(bb), atol)
  double scale;      // beta at a cycle start, eta of a step: what the next basis vector is divided by
  double res0, res1; // |r| at the last cycle start; history[it] at the last close
};

// The tables of a cycle, in doubles from the start of the block; m = restart, entries are pairs (real: the first half)
struct Tables {
  double *c1, *c2;  // the coefficients of the two passes: m entries each
  double *R;        // m x m, column major: column j holds h_0 ... h_(j-1), t
  double *cs, *sn;  // the rotations: c_j (entry), s_j (a double)
  double *g, *y;    // m + 1 and m entries
};
inline size_t table_doubles(int m) { return (size_t)2 * ((size_t)m * 5 + (size_t)m * (size_t)m + 1) + (size_t)m; }
inline Tables tables_at(double *base, int m) {
  Tables T;
  T.c1 = base;
  T.c2 = T.c1 + 2 * m;
  T.R = T.c2 + 2 * m;
  T.cs = T.R + 2 * (size_t)m * (size_t)m;
  T.g = T.cs + 2 * m;
  T.y = T.g + 2 * (m + 1);
  T.sn = T.y + 2 * m;
  return T;
}

__device__ inline Val<1> negated(Val<1> a) { return Val<1>{-a.re}; }
__device__ inline Val<2> negated(Val<2> a) { return Val<2>{-a.re, -a.im}; }

// ---- the vector kernels of a step (dots_kernel and update_kernel: krylov_basis.hpp) ------------------------------------
// r = b - q (q == nullptr: r = b and x = 0); partials of <r,r> and, in the first cycle, of <b,b>
template <int VW, bool FIRST>
__global__ __launch_bounds__(kLanes) void residual_kernel(const GStatus *st, int64_t n, const double *__restrict__ b,
                                                          const double *__restrict__ q, double *__restrict__ x,
                                                          double *__restrict__ r, double *part, int64_t stride) {
  if (!FIRST && (st->done || st->pending)) return;
  chunk_partials<(FIRST ? 2 : 1) * VW>(n, part, stride, [&](int64_t i, double *acc) {
    const Val<VW> bi = load_val<VW>(b, i);
    Val<VW> ri = bi;
    if (q) ri = sub(bi, load_val<VW>(q, i));
    else store_val(x, i, Val<VW>());
    store_val(r, i, ri);
    accumulate(acc, mul(conj_of(ri), ri));
    if (FIRST) accumulate(acc + VW, mul(conj_of(bi), bi));
  });
}

// v = v / *d, part by part: `count` doubles
__global__ __launch_bounds__(kLanes) void divide_kernel(const GStatus *st, int64_t count, const double *d, double *v) {
  if (st->skip) return;
  const double by = *d;
  int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kLanes;
  for (; i < count; i += stride) v[i] = v[i] / by;
}

// The close: u = y_0 v_0, u = u + y_l v_l in ascending l < k; x != nullptr: x = x + u, otherwise u is stored
template <int VW>
__global__ __launch_bounds__(kLanes) void combine_kernel(const GStatus *st, int64_t n, const double *__restrict__ V,
                                                         int64_t ldv, const double *__restrict__ y, double *__restrict__ u,
                                                         double *__restrict__ x) {
  if (st->done) return;
  const int k = st->k;
  if (k == 0) return;
  int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kLanes;
  for (; i < n; i += stride) {
    Val<VW> ui = mul(load_val<VW>(y, 0), load_val<VW>(V, i));
    for (int l = 1; l < k; ++l) ui = add(ui, mul(load_val<VW>(y, l), load_val<VW>(V + (size_t)l * (size_t)ldv * VW, i)));
    if (x) store_val(x, i, add(load_val<VW>(x, i), ui));
    else store_val(u, i, ui);
  }
}

// x = x + z at a close with a preconditioner
template <int VW>
__global__ __launch_bounds__(kLanes) void add_kernel(const GStatus *st, int64_t n, const double *__restrict__ z,
                                                     double *__restrict__ x) {
  if (st->done || st->k == 0) return;
  int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kLanes;
  for (; i < n; i += stride) store_val(x, i, add(load_val<VW>(x, i), load_val<VW>(z, i)));
}

// ---- the scalar kernels: ONE workgroup each ------------------------------------------------------------------------------
// The last level of <r,r> (and <b,b>) at a cycle start, and the cycle's first scalars by lane 0
template <int VW>
__global__ __launch_bounds__(kLanes) void start_kernel(GStatus *st, int first, const double *part, int64_t stride, int count,
                                                       double rtol, double atol, long long max_iter, double *hist,
                                                       double *g) {
  if (st->done) return;
  const int t = threadIdx.x;
  if (!first && st->pending) {  // a breakdown inside the cycle: the close is behind us, the solve ends
    if (t == 0) {
      st->reason = st->pending - 1;
      st->skip = 1;
      st->done = 1;
    }
    return;
  }
  __shared__ double lds[2 * kLanes];
  double f[2] = {0.0, 0.0};  // the real planes: 0 of <r,r>, VW of <b,b>
  for (int i = t; i < count; i += kLanes) f[0] = f[0] + part[i];
  if (first)
    for (int i = t; i < count; i += kLanes) f[1] = f[1] + part[VW * stride + i];
  lane_tree<2>(f, lds);
  if (t != 0) return;
  const double rr = f[0], root = sqrt(rr);
  if (first) {
    const double bb = f[1], by = rtol * sqrt(bb);
    st->bb = bb;
    st->thresh = by > atol ? by : atol;
    st->res1 = root;
    if (hist) hist[0] = root;
  }
  st->rr = rr;
  st->res0 = root;
  int done = 0, reason = 0;
  if (!isfinite(rr) || !isfinite(st->bb)) { done = 1; reason = 3; }
  else if (root <= st->thresh) { done = 1; reason = 0; }
  else if (st->it >= max_iter) { done = 1; reason = 1; }
  if (done) {
    st->reason = reason;
    st->skip = 1;
    st->done = 1;
    return;
  }
  st->scale = root;
  store_val(g, 0, Val<VW>{root});
  st->k = 0;
  st->cycles = st->cycles + 1;
  st->skip = 0;
}

// Step j behind the folds: eta from the partials of <w,w>, h = c1 + c2, the rotations, g, the history and the decisions
template <int VW>
__global__ __launch_bounds__(kLanes) void step_kernel(GStatus *st, int j, int m, const double *part, int count, Tables T,
                                                      long long max_iter, double *hist) {
  if (st->skip) return;
  __shared__ double lds[kLanes];
  const int t = threadIdx.x;
  double f[1] = {0.0};
  for (int i = t; i < count; i += kLanes) f[0] = f[0] + part[i];
  lane_tree<1>(f, lds);
  if (t != 0) return;
  typedef Val<VW> V;
  const double eta = sqrt(f[0]);
  double *h = T.R + 2 * (size_t)j * (size_t)m;  // column j, entries of VW doubles
  auto close = [&](int k, int pending) {
    st->k = k;
    st->pending = pending;
    st->skip = 1;
  };
  bool finite = isfinite(eta);
  for (int i = 0; i <= j; ++i) {
    const V hi = add(load_val<VW>(T.c1, i), load_val<VW>(T.c2, i));
    store_val(h, i, hi);
    finite = finite && is_finite(hi);
  }
  if (!finite) { close(j, 3 + 1); return; }
  for (int i = 0; i < j; ++i) {
    const V c = load_val<VW>(T.cs, i), a = load_val<VW>(h, i), b = load_val<VW>(h, i + 1);
    const double s = T.sn[i];
    store_val(h, i, add(mul(conj_of(c), a), scaled(s, b)));
    store_val(h, i + 1, sub(mul(c, b), scaled(s, a)));
  }
  const V hj = load_val<VW>(h, j);
  const double tt = sqrt(hj.re * hj.re + imag_of(hj) * imag_of(hj) + eta * eta);
  if (tt == 0.0) { close(j, 2 + 1); return; }
  if (!isfinite(tt)) { close(j, 3 + 1); return; }
  const V c = over(hj, tt);
  const double s = eta / tt;
  store_val(T.cs, j, c);
  T.sn[j] = s;
  store_val(h, j, V{tt});
  const V gj = load_val<VW>(T.g, j);
  const V next = negated(scaled(s, gj));
  store_val(T.g, j + 1, next);
  store_val(T.g, j, mul(conj_of(c), gj));
  const long long it = st->it + 1;
  st->it = it;
  const double est = VW == 1 ? fabs(next.re) : sqrt(next.re * next.re + imag_of(next) * imag_of(next));
  if (hist) hist[it] = est;
  st->res1 = est;
  if (est <= st->thresh || eta == 0.0 || j + 1 == m || it >= max_iter) { close(j + 1, 0); return; }
  st->scale = eta;
}

// The back-substitution of a close, by lane 0: y_i = (g_i - sum_l R_il y_l) / R_ii, l ascending
template <int VW>
__global__ __launch_bounds__(64) void solve_kernel(const GStatus *st, int m, Tables T) {
  if (st->done || threadIdx.x != 0) return;
  const int k = st->k;
  for (int i = k - 1; i >= 0; --i) {
    Val<VW> a = load_val<VW>(T.g, i);
    for (int l = i + 1; l < k; ++l) a = sub(a, mul(load_val<VW>(T.R + 2 * (size_t)l * (size_t)m, i), load_val<VW>(T.y, l)));
    store_val(T.y, i, over(a, T.R[2 * (size_t)i * (size_t)m + (size_t)VW * i]));
  }
}

}  // namespace

// k inner products <V[:, i], w> of n entries of vw doubles to d_out; enqueues on s.  Arguments checked by the caller.
int vector_dots(int device, int64_t n, int vw, int k, const double *d_V, int64_t ldv, const double *d_w, double *d_out,
                hipStream_t s) {
  if (n == 0) {
    SPL_HIP(hipMemsetAsync(d_out, 0, (size_t)k * (size_t)vw * sizeof(double), s));  // +0.0, k times
    return SPL_OK;
  }
  DotBlock *block = dot_block_take(device, fold_scratch(n, k * vw));
  if (vw == 1) dots_launch<1>(nullptr, n, k, d_V, ldv, d_w, d_out, block->buf.get(), s);
  else dots_launch<2>(nullptr, n, k, d_V, ldv, d_w, d_out, block->buf.get(), s);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error("vector dots launch", e);
    (void)hipStreamSynchronize(s);
    dot_block_give(block, s, false);
    return SPL_ERROR_device;
  }
  dot_block_give(block, s, true);
  return SPL_OK;
}

// ---- the solver object (the shared part: solver_core.hpp) ---------------------------------------------------------------
struct Gmres : SolverCore {  // work: restart + 3 vectors, the basis v_0 ... v_restart, u, M^-1 u
  int restart;
  Preconditioner pre;
  DBuf<double> tables;
  DBuf<double> hist;  // history[it], grown with the iterations issued (room_for)
  StatusBlock<GStatus> status;
  Gmres(const Matrix *A, int m)
      : SolverCore(kGmresMagic, A, (size_t)m + 3, fold_scratch(A->nrows_local, (m > 1 ? m : 2) * A->vw)), restart(m),
        tables(table_doubles(m)) {
    bytes += table_doubles(m) * sizeof(double) + sizeof(GStatus);
  }
};

// A: whole and square, 1 <= restart <= 128 (the caller checked)
int gmres_create(const Matrix *A, int restart, Gmres **out) {
  *out = new Gmres(A, restart);
  return SPL_OK;
}

void gmres_set_preconditioner(Gmres *G, TriSolver *T1, const double *d_mid, TriSolver *T2) {
  std::lock_guard<std::mutex> hold(G->lock);
  G->pre.set_parts(T1, d_mid, T2);
}

void gmres_set_preconditioner_amg(Gmres *G, Amg *M) {
  std::lock_guard<std::mutex> hold(G->lock);
  G->pre.set_amg(M);
}

namespace {

// One solve's launches; everything is enqueued on s
template <int VW>
struct GRun : LinearRun {
  Gmres *G;
  int m;
  GStatus *st;
  Tables T;

  GRun(Gmres *g, hipStream_t stream, double rt, double at, long long mi, bool history)
      : LinearRun(*g, g->pre, g->hist, stream, rt, at, mi, history), G(g), m(g->restart), st(g->status.device.get()),
        T(tables_at(g->tables.get(), g->restart)) {}

  double *basis(int j) const { return G->vec(j); }
  double *u() const { return G->vec(m + 1); }
  double *mu() const { return G->vec(m + 2); }
  const int *skip() const { return &st->skip; }
  const int *done() const { return &st->done; }
  const GStatus &look() { return LinearRun::look(G->status); }

  // r = b - A x to v_0, its norm, the checks, v_0 = r / beta
  int cycle_start(const double *b, double *x, bool first, int use_x0) {
    const bool product = !first || use_x0;
    if (product) {
      const int e = spmv(x, u());
      if (e != SPL_OK) return e;
    }
    const double *q = product ? u() : nullptr;
    if (first)
      hipLaunchKernelGGL((residual_kernel<VW, true>), dim3(chunked), dim3(kLanes), 0, s, (const GStatus *)st, n, b, q, x,
                         basis(0), scratch, chunks_of(n));
    else
      hipLaunchKernelGGL((residual_kernel<VW, false>), dim3(chunked), dim3(kLanes), 0, s, (const GStatus *)st, n, b, q, x,
                         basis(0), scratch, chunks_of(n));
    const Partials P = middle_levels(done(), n, (first ? 2 : 1) * VW, scratch, s);
    hipLaunchKernelGGL((start_kernel<VW>), dim3(1), dim3(kLanes), 0, s, st, first ? 1 : 0, P.p, P.stride, P.count, rtol,
                       atol, max_iter, hist.get(), T.g);
    hipLaunchKernelGGL(divide_kernel, dim3(flat), dim3(kLanes), 0, s, (const GStatus *)st, n * VW,
                       (const double *)&st->scale, basis(0));
    launches += P.middle + 3;
    return SPL_OK;
  }

  int step(int j) {
    const double *z = basis(j);
    int e;
    if (pre.set()) {
      if ((e = apply<VW>(basis(j), mu(), skip())) != SPL_OK) return e;
      z = mu();
    }
    double *w = basis(j + 1);
    if ((e = spmv(z, w)) != SPL_OK) return e;
    const Partials P = orthogonalise_twice<VW>(skip(), n, j + 1, basis(0), w, T.c1, T.c2, scratch, chunked, s, &launches);
    hipLaunchKernelGGL((step_kernel<VW>), dim3(1), dim3(kLanes), 0, s, st, j, m, P.p, P.count, T, max_iter, hist.get());
    hipLaunchKernelGGL(divide_kernel, dim3(flat), dim3(kLanes), 0, s, (const GStatus *)st, n * VW,
                       (const double *)&st->scale, w);
    launches += 2;
    return SPL_OK;
  }

  int close(double *x) {
    hipLaunchKernelGGL((solve_kernel<VW>), dim3(1), dim3(64), 0, s, (const GStatus *)st, m, T);
    ++launches;
    if (!pre.set()) {
      hipLaunchKernelGGL((combine_kernel<VW>), dim3(flat), dim3(kLanes), 0, s, (const GStatus *)st, n,
                         (const double *)basis(0), n, (const double *)T.y, (double *)nullptr, x);
      ++launches;
      return SPL_OK;
    }
    hipLaunchKernelGGL((combine_kernel<VW>), dim3(flat), dim3(kLanes), 0, s, (const GStatus *)st, n,
                       (const double *)basis(0), n, (const double *)T.y, u(), (double *)nullptr);
    const int e = apply<VW>(u(), mu(), done());
    if (e != SPL_OK) return e;
    hipLaunchKernelGGL((add_kernel<VW>), dim3(flat), dim3(kLanes), 0, s, (const GStatus *)st, n, (const double *)mu(), x);
    launches += 2;
    return SPL_OK;
  }

  int solve(const double *b, double *x, int use_x0, int check_every, GStatus *last) {
    const long long every = check_every > 0 ? check_every : 1;
    int e;
    SPL_HIP(hipMemsetAsync(st, 0, sizeof(GStatus), s));
    room_for(hist, every * m + 1, 0, max_iter);
    if ((e = cycle_start(b, x, true, use_x0)) != SPL_OK) return e;
    if ((e = launch_status("gmres start")) != SPL_OK) return e;
    // One look before the first cycle: a start that is already good enough (or not finite) costs no cycle issued for
    // nothing.  A cycle completes an iteration or ends the solve, and max_iter iterations end it: max_iter + 1 cycles
    // at most
    bool ended = look().done != 0;
    for (long long issued = 0; !ended;) {
      for (int j = 0; j < m; ++j)
        if ((e = step(j)) != SPL_OK) return e;
      if ((e = close(x)) != SPL_OK) return e;
      if ((e = cycle_start(b, x, false, 1)) != SPL_OK) return e;
      if ((e = launch_status("gmres cycle")) != SPL_OK) return e;
      ++issued;
      if (issued % every == 0) {
        const GStatus &now = look();
        if (now.done) break;
        room_for(hist, now.it + every * m + 1, now.it + 1, max_iter);
      }
    }
    *last = look();
    return SPL_OK;
  }
};

template <int VW>
int solve_width(Gmres *G, const double *d_b, double *d_x, int use_x0, double rtol, double atol, int64_t max_iter,
                int check_every, int64_t result[6], double *history, double residual[2], hipStream_t s) {
  GRun<VW> run(G, s, rtol, atol, (long long)max_iter, history != nullptr);
  GStatus last;
  memset(&last, 0, sizeof(last));
  const int e = run.solve(d_b, d_x, use_x0, check_every, &last);
  if (e != SPL_OK) {
    (void)hipStreamSynchronize(s);
    return e;
  }
  result[0] = last.it;
  result[1] = last.done ? last.reason : 1;
  result[2] = last.cycles;
  result[3] = run.spmvs;
  result[4] = run.applications;
  result[5] = 0;
  residual[0] = last.res0;
  residual[1] = last.res1;
  if (history) {
    SPL_HIP(hipMemcpyAsync(history, run.hist.get(), ((size_t)last.it + 1) * sizeof(double), hipMemcpyDeviceToHost, s));
    SPL_HIP(hipStreamSynchronize(s));
  }
  G->last_rounds = last.it;
  G->last_launches = run.launches;
  ++G->solves;
  return SPL_OK;
}

}  // namespace

// arguments checked by the caller; n > 0.  Enqueues on s and synchronises it: the result is read back.
int gmres_solve(Gmres *G, const double *d_b, double *d_x, int use_x0, double rtol, double atol, int64_t max_iter,
                int check_every, int64_t result[6], double *history, double residual[2], hipStream_t s) {
  std::lock_guard<std::mutex> hold(G->lock);
  if (G->vw == 1)
    return solve_width<1>(G, d_b, d_x, use_x0, rtol, atol, max_iter, check_every, result, history, residual, s);
  return solve_width<2>(G, d_b, d_x, use_x0, rtol, atol, max_iter, check_every, result, history, residual, s);
}

void gmres_info(Gmres *G, int64_t info[8]) {
  std::lock_guard<std::mutex> hold(G->lock);
  G->fill_info(info, G->restart, G->pre.flags());
}

void gmres_delete(Gmres *G) { delete_object(G); }

}  // namespace spl

// eigsh.hip — thick-restart Lanczos with full reorthogonalisation on device handles, Double and packed Complex Double
// (real symmetric and complex Hermitian), and the in-place basis rotation its restart is built on
// (spl_vector_rotate_dev).
//
// The arithmetic is the fold of krylov_fold.hpp and the sequence of include/sparse_linear_hip.h ("thick-restart
// Lanczos").  A step is a GMRES step: the product, classical Gram-Schmidt done twice with the one-pass kernels of
// krylov_basis.hpp, the norm.  In direct mode no scalar leaves the device inside a cycle: ONE workgroup behind the folds
// (step_kernel) writes alpha_j and beta_j into a table and sets `skip` when the cycle ends early; the host issues every
// step and each kernel returns on `skip`.  In inverse mode the product is a solve by a spl_krylov object, which
// synchronises anyway, and the host reads the status block behind every step.
//
// The close is the host's: one synchronisation per cycle brings the two tables down, the projected matrix (an arrow head
// from the restart and a tridiagonal tail) goes through the Ritz step of ritz_jacobi.hpp (cyclic Jacobi and the order, in
// plain C++; -ffp-contract=off: a product and a sum are rounded apart on the host too), and the restart
// V[:, :k] <- V Y is the rotate kernel IN PLACE: a row tile of the basis is staged in LDS, so every input of a row is
// read before any output of that row is written, and no second basis exists.  No kernel waits for another workgroup,
// there is no floating-point atomic and no captured graph.
#include <algorithm>
#include <cmath>
#include <vector>

#include "krylov_basis.hpp"
#include "ritz_jacobi.hpp"
#include "solver_core.hpp"

namespace spl {

namespace {

constexpr int kRotateCols = 4;              // output columns a lane carries through one walk over the tile's columns
constexpr int kRotateRowsLog2 = 6;          // rows of a tile: 64; SPL_EIGSH_ROTATE_ROWS = 16, 32, 64
constexpr size_t kRotateLds = 64 * 1024;    // bytes of LDS a tile may take

// ---- V[:, :k] <- V Y ---------------------------------------------------------------------------------------------------
// A workgroup takes tiles of R = 2^rows_log2 consecutive rows.  Load: lane t takes row t mod R of the columns t / R,
// t / R + 256 / R, ...: consecutive lanes read consecutive rows of a column.  The tile lies in LDS plane by plane,
// tile[(l * VW + p) * R + r], so the R lanes that read column l in the product read consecutive doubles (no bank
// conflict; lanes of another column group read the same words, a broadcast).  Product: the lane keeps its row and takes
// the output columns g, g + G, ... (G = 256 / R), kRotateCols of them per walk over l, each
// x = Y[0][i] v_0; x = x + Y[l][i] v_l ascending, a product and a sum per term and part.  V and out may be the same
// array: a tile's loads are all in front of the barrier, its stores behind it, and no other workgroup touches its rows.
// WAVE (R == 64): a wavefront is one column group, so its output columns and the entries of Y it needs are the same in
// every lane, and Y is read through the scalar cache instead of one vector load per lane and term.
// YZ (spl_vector_rotate_z_dev, VW == 2): Y holds packed pairs and a term is x = x + Y[l][i] v_l with Data.Complex's
// product, (ac - bd, ad + bc) for Y = a + bi and v = c + di, each operation rounded once.
template <int VW, bool WAVE, bool YZ = false>
__global__ __launch_bounds__(kLanes) void rotate_kernel(int64_t n, int m, int k, int rows_log2, const double *V,
                                                        int64_t ldv, const double *__restrict__ Y, int ldy, double *out,
                                                        int64_t ldo) {
  extern __shared__ double tile[];
  constexpr int kTerms = WAVE ? 2 : 4;  // terms per round of the walk: by four the scalar registers of WAVE do not fit
  const int R = 1 << rows_log2, t = threadIdx.x, r = t & (R - 1), G = kLanes >> rows_log2;
  const int g = WAVE ? __builtin_amdgcn_readfirstlane(t >> rows_log2) : t >> rows_log2;
  const int64_t ntiles = (n + R - 1) >> rows_log2;
  for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
    const int64_t row = (tl << rows_log2) + r;
    const bool live = row < n;
    for (int l = g; l < m; l += G) {
      const Val<VW> v = live ? load_val<VW>(V + (size_t)l * (size_t)ldv * VW, row) : Val<VW>();
      tile[(size_t)(l * VW) * R + r] = v.re;
      if (VW == 2) tile[(size_t)(l * VW + 1) * R + r] = imag_of(v);
    }
    __syncthreads();
    for (int i0 = g; i0 < k; i0 += kRotateCols * G) {
      const double *y[kRotateCols];
      double acc[kRotateCols * VW];
#pragma unroll
      for (int c = 0; c < kRotateCols; ++c) {
        const int col = i0 + c * G;
        y[c] = Y + (size_t)(col < k ? col : i0) * (size_t)ldy * (YZ ? 2 : 1);  // past k: computed again, never stored
      }
      if constexpr (YZ) {
        const double a = tile[r], b = tile[(size_t)R + r];
#pragma unroll
        for (int c = 0; c < kRotateCols; ++c) {
          const Val<2> x = mul(Val<2>{y[c][0], y[c][1]}, Val<2>{a, b});
          acc[c * 2] = x.re;
          acc[c * 2 + 1] = x.im;
        }
#pragma unroll kTerms
        for (int l = 1; l < m; ++l) {
          const double a = tile[(size_t)(l * 2) * R + r], b = tile[(size_t)(l * 2 + 1) * R + r];
#pragma unroll
          for (int c = 0; c < kRotateCols; ++c) {
            const Val<2> x = mul(Val<2>{y[c][2 * l], y[c][2 * l + 1]}, Val<2>{a, b});
            acc[c * 2] = acc[c * 2] + x.re;
            acc[c * 2 + 1] = acc[c * 2 + 1] + x.im;
          }
        }
      } else {
#pragma unroll
        for (int p = 0; p < VW; ++p) {
          const double a = tile[(size_t)p * R + r];
#pragma unroll
          for (int c = 0; c < kRotateCols; ++c) acc[c * VW + p] = y[c][0] * a;
        }
#pragma unroll kTerms
        for (int l = 1; l < m; ++l) {
#pragma unroll
          for (int p = 0; p < VW; ++p) {
            const double a = tile[(size_t)(l * VW + p) * R + r];
#pragma unroll
            for (int c = 0; c < kRotateCols; ++c) acc[c * VW + p] = acc[c * VW + p] + y[c][l] * a;
          }
        }
      }
      if (live) {
#pragma unroll
        for (int c = 0; c < kRotateCols; ++c) {
          const int col = i0 + c * G;
          if (col < k) store_val(out + (size_t)col * (size_t)ldo * VW, row, from_planes<VW>(acc + c * VW, 0));
        }
      }
    }
    __syncthreads();  // the tile is written again for the workgroup's next rows
  }
}

// rows of a tile: the knob, halved until the tile fits; a function of m and the value width alone
int rotate_rows_log2(int m, int vw) {
  const char *e = getenv("SPL_EIGSH_ROTATE_ROWS");
  const long v = e ? atol(e) : 0;
  int lg = v == 16 ? 4 : v == 32 ? 5 : v == 64 ? 6 : kRotateRowsLog2;
  while (lg > 4 && ((size_t)m * (size_t)vw * sizeof(double) << lg) > kRotateLds) --lg;
  return lg;
}

// n > 0; 1 <= k <= m <= 128.  One launch on s.  y_complex: Y holds packed pairs (vw == 2 only)
void rotate_launch(int64_t n, int vw, int m, int k, const double *V, int64_t ldv, const double *Y, int ldy,
                   double *out, int64_t ldo, hipStream_t s, bool y_complex = false) {
  const int lg = rotate_rows_log2(m, vw);
  const size_t lds = (size_t)m * (size_t)vw * sizeof(double) << lg;
  const int64_t tiles = (n + ((int64_t)1 << lg) - 1) >> lg, cap = chunk_grid_cap();
  const dim3 grid((unsigned)(tiles < cap ? tiles : cap)), block(kLanes);
  if (y_complex && lg == 6)
    hipLaunchKernelGGL((rotate_kernel<2, true, true>), grid, block, lds, s, n, m, k, lg, V, ldv, Y, ldy, out, ldo);
  else if (y_complex)
    hipLaunchKernelGGL((rotate_kernel<2, false, true>), grid, block, lds, s, n, m, k, lg, V, ldv, Y, ldy, out, ldo);
  else if (vw == 1 && lg == 6)
    hipLaunchKernelGGL((rotate_kernel<1, true>), grid, block, lds, s, n, m, k, lg, V, ldv, Y, ldy, out, ldo);
  else if (vw == 1)
    hipLaunchKernelGGL((rotate_kernel<1, false>), grid, block, lds, s, n, m, k, lg, V, ldv, Y, ldy, out, ldo);
  else if (lg == 6)
    hipLaunchKernelGGL((rotate_kernel<2, true>), grid, block, lds, s, n, m, k, lg, V, ldv, Y, ldy, out, ldo);
  else
    hipLaunchKernelGGL((rotate_kernel<2, false>), grid, block, lds, s, n, m, k, lg, V, ldv, Y, ldy, out, ldo);
}

// ---- the status block and the tables -------------------------------------------------------------------------------------
struct EStatus {
  int skip;       // the cycle is closed (eta == 0) or the solve is over (pending): the kernels of a step return
  int pending;    // reason + 1 of what ends the solve
  int mprime;     // columns of the cycle so far: j + 1 behind step j
  int spare;
  long long ops;  // applications of the operator
  double scale;   // eta: what the next basis vector is divided by
  double eta0;    // the norm of the start
};

// in doubles from the start of the block; m = ncv
struct ETables {
  double *alpha, *beta;  // m each; with `res` the part the host reads at a close and at the end
  double *res;           // m: |r_i|^2 of the pairs returned
  double *c1, *c2;       // the coefficients of the two passes: m entries each
  double *Y;             // m x m, column major
};
inline size_t etable_doubles(int m) { return (size_t)7 * (size_t)m + (size_t)m * (size_t)m; }
inline ETables etables_at(double *base, int m) {
  ETables T;
  T.c1 = base;  // packed pairs are loaded whole: 16-byte aligned
  T.c2 = T.c1 + 2 * m;
  T.alpha = T.c2 + 2 * m;
  T.beta = T.alpha + m;
  T.res = T.beta + m;
  T.Y = T.res + m;
  return T;
}

// ---- the vector kernels (norm_kernel and residual_kernel: krylov_basis.hpp) -------------------------------------------
// out = in / *d, part by part: `count` doubles; in and out may be the same array
__global__ __launch_bounds__(kLanes) void divide_kernel(const int *stop, int64_t count, const double *d, const double *in,
                                                        double *out) {
  if (*stop) return;
  const double by = *d;
  int64_t i = (int64_t)blockIdx.x * kLanes + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kLanes;
  for (; i < count; i += stride) out[i] = in[i] / by;
}

// ---- the scalar kernels: ONE workgroup each ------------------------------------------------------------------------------
// eta = sqrt(Re<v0,v0>) from the last partials, and what it decides
__global__ __launch_bounds__(kLanes) void start_kernel(EStatus *st, const double *part, int count) {
  const double sum = sum_partials(part, count);
  if (threadIdx.x != 0) return;
  const double eta = sqrt(sum);
  st->eta0 = eta;
  if (!isfinite(eta)) {
    st->pending = 3 + 1;
    st->skip = 1;
  } else if (eta == 0.0) {
    st->pending = 2 + 1;
    st->skip = 1;
  } else {
    st->scale = eta;
  }
}

// Step j behind the folds: eta from the partials of <w,w>, alpha_j = Re(c1_j + c2_j), the two tables and the decisions
template <int VW>
__global__ __launch_bounds__(kLanes) void step_kernel(EStatus *st, int j, const double *part, int count, ETables T) {
  if (st->skip) return;
  const double sum = sum_partials(part, count);
  if (threadIdx.x != 0) return;
  const double eta = sqrt(sum);
  const double alpha = add(load_val<VW>(T.c1, j), load_val<VW>(T.c2, j)).re;
  T.alpha[j] = alpha;
  T.beta[j] = eta;
  st->ops = st->ops + 1;
  if (!isfinite(alpha) || !isfinite(eta)) {
    st->pending = 3 + 1;
    st->skip = 1;
    return;
  }
  st->mprime = j + 1;
  if (eta == 0.0) {
    st->skip = 1;
    return;
  }
  st->scale = eta;
}

}  // namespace

// V[:, :k] <- V Y (d_out == nullptr) or out = V Y; enqueues on s.  Arguments checked by the caller.
int vector_rotate(int64_t n, int vw, int m, int k, double *d_V, int64_t ldv, const double *d_Y, int ldy, double *d_out,
                  int64_t ldo, hipStream_t s, bool y_complex) {
  if (n == 0) return SPL_OK;
  rotate_launch(n, vw, m, k, d_V, ldv, d_Y, ldy, d_out ? d_out : d_V, d_out ? ldo : ldv, s, y_complex);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_last_error("vector rotate launch", e);
    (void)hipStreamSynchronize(s);
    return SPL_ERROR_device;
  }
  return SPL_OK;
}

// ---- the solver object (the shared part: solver_core.hpp) ---------------------------------------------------------------
struct Eigsh : SolverCore {  // work: ncv + 2 vectors, the basis v_0 ... v_ncv and A x of the residuals
  int ncv;
  Krylov *K = nullptr;  // borrowed; set: the operator is (A - sigma I)^-1 by K
  double sigma = 0.0, rtol = 0.0, atol = 0.0;
  int64_t max_iter = 0;
  DBuf<double> tables;
  StatusBlock<EStatus> status;  // behind the pinned copy: alpha, beta and res, and the ncv x ncv doubles that go up
  Eigsh(const Matrix *A, int m)
      : SolverCore(kEigshMagic, A, (size_t)m + 2, fold_scratch(A->nrows_local, m * A->vw)), ncv(m),
        tables(etable_doubles(m)), status(((size_t)3 * m + (size_t)m * m) * sizeof(double)) {
    bytes += etable_doubles(m) * sizeof(double) + sizeof(EStatus);
  }
  double *host_tables() const { return reinterpret_cast<double *>(status.pinned + 1); }
  double *host_y() const { return host_tables() + 3 * ncv; }
};

// A: whole, square and Hermitian, 2 <= ncv <= 128 (the caller checked)
int eigsh_create(const Matrix *A, int ncv, Eigsh **out) {
  *out = new Eigsh(A, ncv);
  return SPL_OK;
}

void eigsh_set_inverse(Eigsh *E, Krylov *K, double sigma, double rtol, double atol, int64_t max_iter) {
  std::lock_guard<std::mutex> hold(E->lock);
  E->K = K;
  E->sigma = K ? sigma : 0.0;
  E->rtol = rtol;
  E->atol = atol;
  E->max_iter = max_iter;
}

namespace {

// One solve's launches; everything is enqueued on s
template <int VW>
struct ERun : RunCore {
  Eigsh *E;
  int m;  // ncv
  EStatus *st;
  ETables T;
  int64_t inner = 0;

  ERun(Eigsh *e, hipStream_t stream)
      : RunCore(*e, stream), E(e), m(e->ncv), st(e->status.device.get()), T(etables_at(e->tables.get(), e->ncv)) {}

  double *basis(int j) const { return E->vec(j); }
  double *product() const { return E->vec(m + 1); }
  const int *skip() const { return &st->skip; }

  // tables: alpha, beta and res come down beside the status block
  const EStatus &look(bool tables) {
    return RunCore::look(E->status, [&] {
      if (tables)
        SPL_HIP(hipMemcpyAsync(E->host_tables(), T.alpha, (size_t)3 * m * sizeof(double), hipMemcpyDeviceToHost, s));
    });
  }

  void start(const double *v0) {
    hipLaunchKernelGGL((norm_kernel<VW>), dim3(chunked), dim3(kLanes), 0, s, n, v0, scratch);
    const Partials P = last_level();
    hipLaunchKernelGGL(start_kernel, dim3(1), dim3(kLanes), 0, s, st, P.p, P.count);
    hipLaunchKernelGGL(divide_kernel, dim3(flat), dim3(kLanes), 0, s, skip(), n * VW, (const double *)&st->scale, v0,
                       basis(0));
    launches += 3;
  }

  // w = OP v_j to slot j + 1; *failed: the inner solve did not converge
  int apply(int j, bool *failed) {
    if (!E->K) {
      ++launches;
      return launch_spmv(E->A, basis(j), basis(j + 1), 0, s);
    }
    int64_t result[4] = {0, 0, 0, 0};
    const int e = krylov_solve(E->K, basis(j), basis(j + 1), 0, E->rtol, E->atol, E->max_iter, 0, result, nullptr, s);
    if (e != SPL_OK) return e;
    inner += result[0];
    *failed = result[1] != 0;
    return SPL_OK;
  }

  void orthogonalise(int j) {
    double *w = basis(j + 1);
    const Partials P = orthogonalise_twice<VW>(skip(), n, j + 1, basis(0), w, T.c1, T.c2, scratch, chunked, s, &launches);
    hipLaunchKernelGGL((step_kernel<VW>), dim3(1), dim3(kLanes), 0, s, st, j, P.p, P.count, T);
    hipLaunchKernelGGL(divide_kernel, dim3(flat), dim3(kLanes), 0, s, skip(), n * VW, (const double *)&st->scale,
                       (const double *)w, w);
    launches += 2;
  }

  // Y[:, order[0 .. cols)] of the m' x m' host matrix to the device table, leading dimension m'
  void upload(const std::vector<double> &Y, const std::vector<int> &order, int mp, int cols) {
    double *h = E->host_y();
    for (int c = 0; c < cols; ++c)
      for (int r = 0; r < mp; ++r) h[(size_t)c * mp + r] = Y[(size_t)r * mp + order[c]];
    SPL_HIP(hipMemcpyAsync(T.Y, h, (size_t)cols * mp * sizeof(double), hipMemcpyHostToDevice, s));
  }

  // X = V Y[:, :pairs], the values and the residual norms; synchronises
  int finish(const std::vector<double> &Y, const std::vector<int> &order, const std::vector<double> &theta, int mp,
             int pairs, double *values, double *d_vectors, int64_t ldx, double *residuals) {
    if (pairs == 0) return SPL_OK;
    upload(Y, order, mp, pairs);
    rotate_launch(n, VW, mp, pairs, basis(0), n, T.Y, mp, d_vectors, ldx, s);
    ++launches;
    for (int i = 0; i < pairs; ++i) {
      values[i] = E->K ? E->sigma + 1.0 / theta[i] : theta[i];
      const double *x = d_vectors + (size_t)i * (size_t)ldx * VW;
      const int e = launch_spmv(E->A, x, product(), 0, s);
      if (e != SPL_OK) return e;
      hipLaunchKernelGGL((residual_kernel<VW>), dim3(chunked), dim3(kLanes), 0, s, n, (const double *)product(), x,
                         values[i], (double *)nullptr, scratch);
      launches += 2;
      fold_to(T.res + i);
    }
    const int e = launch_status("eigsh finish");
    if (e != SPL_OK) return e;
    look(true);
    const double *res = E->host_tables() + 2 * m;
    for (int i = 0; i < pairs; ++i) residuals[i] = sqrt(res[i]);
    return SPL_OK;
  }

  int solve(int nev, int which, double tol, double atol, int64_t max_restarts, const double *d_v0, double *values,
            double *d_vectors, int64_t ldx, double *residuals, int64_t result[6], double *history) {
    int e;
    SPL_HIP(hipMemsetAsync(st, 0, sizeof(EStatus), s));
    start(d_v0);
    if ((e = launch_status("eigsh start")) != SPL_OK) return e;
    EStatus now = look(false);
    if (history) history[0] = now.eta0;
    int64_t cycles = 0, ops = 0, sweeps_most = 0;
    auto done = [&](int reason, int pairs) {
      result[0] = reason;
      result[1] = cycles;
      result[2] = ops;
      result[3] = pairs;
      result[4] = inner;
      result[5] = sweeps_most;
      return SPL_OK;
    };
    if (now.pending) return done(now.pending - 1, 0);
    int k = 0;
    std::vector<double> theta, kept;  // theta_i and s_i of the restart, i < k
    std::vector<double> Tm, Y, est;
    std::vector<int> order;
    for (;;) {
      bool failed = false;
      for (int j = k; j < m && !failed; ++j) {
        if ((e = apply(j, &failed)) != SPL_OK) return e;
        if (failed) break;
        orthogonalise(j);
        if (E->K && look(false).skip) break;  // the product is a solve of its own: it does not read `skip`
      }
      if ((e = launch_status("eigsh cycle")) != SPL_OK) return e;
      now = look(true);
      ops = now.ops;
      if (failed) return done(4, 0);
      if (now.pending) return done(now.pending - 1, 0);
      const int mp = now.mprime;
      const bool invariant = now.skip != 0;  // eta == 0 closed the cycle
      const double *alpha = E->host_tables(), *beta = alpha + m;
      Tm.assign((size_t)mp * mp, 0.0);
      Y.assign((size_t)mp * mp, 0.0);
      for (int i = 0; i < k; ++i) {
        Tm[(size_t)i * mp + i] = theta[i];
        Tm[(size_t)i * mp + k] = Tm[(size_t)k * mp + i] = kept[i];
      }
      for (int j = k; j < mp; ++j) {
        Tm[(size_t)j * mp + j] = alpha[j];
        if (j < mp - 1) Tm[(size_t)j * mp + j + 1] = Tm[(size_t)(j + 1) * mp + j] = beta[j];
      }
      const double last = beta[mp - 1];
      order.resize(mp);
      const int sweeps = ritz_step(mp, 1, which, Tm.data(), Y.data(), order.data());
      if (sweeps < 0) return done(3, 0);
      ++cycles;
      if (sweeps > sweeps_most) sweeps_most = sweeps;
      auto value = [&](int i) { return Tm[(size_t)i * mp + i]; };
      const int pairs = nev < mp ? nev : mp;
      est.assign(mp, 0.0);
      double worst = 0.0;
      bool converged = true;
      for (int i = 0; i < mp; ++i) {
        est[i] = fabs(last * Y[(size_t)(mp - 1) * mp + order[i]]);
        if (i >= pairs) continue;
        if (est[i] > worst) worst = est[i];
        const double bound = tol * fabs(value(order[i]));
        converged = converged && est[i] <= (bound > atol ? bound : atol);
      }
      if (history) history[cycles] = worst;
      int reason = -1;
      if (invariant) reason = mp >= nev ? 0 : 2;
      else if (converged) reason = 0;
      else if (cycles >= max_restarts) reason = 1;
      if (reason >= 0) {
        std::vector<double> sorted(pairs);
        for (int i = 0; i < pairs; ++i) sorted[i] = value(order[i]);
        if ((e = finish(Y, order, sorted, mp, pairs, values, d_vectors, ldx, residuals)) != SPL_OK) return e;
        return done(reason, pairs);
      }
      // ---- the restart: k Ritz vectors and v_(m'), the arrow head theta_i, s_i
      const int half = nev + (mp - nev) / 2;
      k = half < mp - 1 ? half : mp - 1;
      upload(Y, order, mp, k);
      rotate_launch(n, VW, mp, k, basis(0), n, T.Y, mp, basis(0), n, s);
      SPL_HIP(hipMemcpyAsync(basis(k), basis(mp), (size_t)n * VW * sizeof(double), hipMemcpyDeviceToDevice, s));
      launches += 2;
      theta.resize(k);
      kept.resize(k);
      for (int i = 0; i < k; ++i) {
        theta[i] = value(order[i]);
        kept[i] = last * Y[(size_t)(mp - 1) * mp + order[i]];
      }
    }
  }
};

}  // namespace

// arguments checked by the caller; n > 0.  Enqueues on s and synchronises it: the outcome is read back.
int eigsh_solve(Eigsh *E, int nev, int which, double tol, double atol, int64_t max_restarts, const double *d_v0,
                double *values, double *d_vectors, int64_t ldx, double *residuals, int64_t result[6], double *history,
                hipStream_t s) {
  std::lock_guard<std::mutex> hold(E->lock);
  return E->solve_and_record(s, result + 1, [&](auto width, int64_t *launches) {
    ERun<decltype(width)::value> run(E, s);
    const int e = run.solve(nev, which, tol, atol, max_restarts, d_v0, values, d_vectors, ldx, residuals, result, history);
    *launches = run.launches;
    return e;
  });
}

void eigsh_info(Eigsh *E, int64_t info[8]) {
  std::lock_guard<std::mutex> hold(E->lock);
  E->fill_info(info, E->ncv, E->K ? 2 : 0);
}

int eigsh_ncv(const Eigsh *E) { return E->ncv; }

void eigsh_delete(Eigsh *E) { delete_object(E); }

}  // namespace spl

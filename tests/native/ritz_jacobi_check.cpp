// Runs the two cyclic Jacobi rules of csrc/ritz_jacobi.hpp (real symmetric, complex Hermitian) on fixed matrices of the
// orders 1, 2, 3, 17 and 60, checks what they leave (no coupling, an orthonormal Y, Y diag(theta) Y^H = T to rounding
// level) and prints every theta and every entry of Y as hexadecimal floats, for tests/test_ritz_jacobi.py to compare
// with the restatement bit by bit.  Then the Ritz step both eigensolvers call (ritz_step: the rule, the refusal of what
// is not finite, the stable order) for each of the three orders on the orders 1, 2, 3 and 17, on matrices with equal
// values and on matrices holding a NaN or an infinity.  Built with the address and undefined-behaviour sanitizers;
// -ffp-contract=off, as the library is.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ritz_jacobi.hpp"

namespace {

uint64_t state = 0x243F6A8885A308D3ull;
double next_entry() {  // in [-0.5, 0.5): tests/test_ritz_jacobi.py draws the same numbers
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(state >> 11) * 0x1p-53 - 0.5;
}

int bad = 0;
void expect(bool ok, const char *what, int m) {
  if (!ok) {
    ++bad;
    std::fprintf(stderr, "order %d: %s\n", m, what);
  }
}

void run_real(int m) {
  std::vector<double> T((size_t)m * m), T0, Y((size_t)m * m);
  for (int r = 0; r < m; ++r)
    for (int c = r; c < m; ++c) T[(size_t)r * m + c] = T[(size_t)c * m + r] = next_entry();
  T0 = T;
  const int sweeps = spl::ritz_jacobi_real(m, T.data(), Y.data());
  expect(sweeps >= 0 && sweeps <= 12, "sweeps", m);
  double norm = 0.0;
  for (double v : T0) norm += v * v;
  norm = std::sqrt(norm);
  const double tol = 64.0 * m * 0x1p-53 * (norm > 0.0 ? norm : 1.0), unit = 64.0 * m * 0x1p-53;
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < m; ++c) {
      if (r != c) expect(T[(size_t)r * m + c] == 0.0, "a coupling is left", m);
      double dot = 0.0, back = 0.0;
      for (int l = 0; l < m; ++l) {
        dot += Y[(size_t)l * m + r] * Y[(size_t)l * m + c];
        back += Y[(size_t)r * m + l] * T[(size_t)l * m + l] * Y[(size_t)c * m + l];
      }
      expect(std::fabs(dot - (r == c ? 1.0 : 0.0)) <= unit, "Y is not orthonormal", m);
      expect(std::fabs(back - T0[(size_t)r * m + c]) <= tol, "Y theta Y^T is not T", m);
    }
  std::printf("real %d %d", m, sweeps);
  for (int i = 0; i < m; ++i) std::printf(" %a", T[(size_t)i * m + i]);
  for (double v : Y) std::printf(" %a", v);
  std::printf("\n");
}

void run_hermitian(int m) {
  std::vector<double> T((size_t)2 * m * m), T0, Y((size_t)2 * m * m);
  for (int r = 0; r < m; ++r)
    for (int c = r; c < m; ++c) {
      const double re = next_entry(), im = r == c ? 0.0 : next_entry();
      T[2 * ((size_t)r * m + c)] = T[2 * ((size_t)c * m + r)] = re;
      T[2 * ((size_t)r * m + c) + 1] = im;
      T[2 * ((size_t)c * m + r) + 1] = r == c ? 0.0 : -im;
    }
  T0 = T;
  const int sweeps = spl::ritz_jacobi_hermitian(m, T.data(), Y.data());
  expect(sweeps >= 0 && sweeps <= 12, "sweeps", m);
  double norm = 0.0;
  for (double v : T0) norm += v * v;
  norm = std::sqrt(norm);
  const double tol = 64.0 * m * 0x1p-53 * (norm > 0.0 ? norm : 1.0), unit = 64.0 * m * 0x1p-53;
  auto re = [m](const std::vector<double> &M, int r, int c) { return M[2 * ((size_t)r * m + c)]; };
  auto im = [m](const std::vector<double> &M, int r, int c) { return M[2 * ((size_t)r * m + c) + 1]; };
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < m; ++c) {
      if (r != c) expect(re(T, r, c) == 0.0 && im(T, r, c) == 0.0, "a coupling is left", m);
      double dr = 0.0, di = 0.0, br = 0.0, bi = 0.0;
      for (int l = 0; l < m; ++l) {  // conj(Y_lr) Y_lc, and Y_rl theta_l conj(Y_cl)
        dr += re(Y, l, r) * re(Y, l, c) + im(Y, l, r) * im(Y, l, c);
        di += re(Y, l, r) * im(Y, l, c) - im(Y, l, r) * re(Y, l, c);
        const double th = re(T, l, l);
        br += th * (re(Y, r, l) * re(Y, c, l) + im(Y, r, l) * im(Y, c, l));
        bi += th * (im(Y, r, l) * re(Y, c, l) - re(Y, r, l) * im(Y, c, l));
      }
      expect(std::fabs(dr - (r == c ? 1.0 : 0.0)) <= unit && std::fabs(di) <= unit, "Y is not unitary", m);
      expect(std::fabs(br - re(T0, r, c)) <= tol && std::fabs(bi - (r == c ? 0.0 : im(T0, r, c))) <= tol,
             "Y theta Y^H is not T", m);
    }
  std::printf("hermitian %d %d", m, sweeps);
  for (int i = 0; i < m; ++i) std::printf(" %a", re(T, i, i));
  for (double v : Y) std::printf(" %a", v);
  std::printf("\n");
}

// ritz_step on T (width 1: m x m doubles; 2: packed pairs), which it overwrites: the line has the sweeps (-1: refused,
// and nothing behind it), every theta and the order, its indices printed as floats like every other number of a line
void run_step(const char *name, int m, int width, int which, std::vector<double> T) {
  std::vector<double> Y(T.size());
  std::vector<int> order(m, -1);
  const int sweeps = spl::ritz_step(m, width, which, T.data(), Y.data(), order.data());
  std::printf("step-%s-%d %d %d", name, which, m, sweeps);
  if (sweeps >= 0) {
    std::vector<bool> seen(m, false);
    for (int i = 0; i < m; ++i) {
      expect(order[i] >= 0 && order[i] < m && !seen[order[i]], "the order is not a permutation", m);
      if (order[i] >= 0 && order[i] < m) seen[order[i]] = true;
    }
    for (int i = 0; i < m; ++i) std::printf(" %a", T[((size_t)i * m + i) * width]);
    for (int i = 0; i < m; ++i) std::printf(" %a", (double)order[i]);
  } else {
    for (int i = 0; i < m; ++i) expect(order[i] == -1, "a refused step wrote the order", m);
  }
  std::printf("\n");
}

void run_steps(int which) {
  const int orders[4] = {1, 2, 3, 17};
  for (int m : orders) {
    std::vector<double> T((size_t)m * m);
    for (int r = 0; r < m; ++r)
      for (int c = r; c < m; ++c) T[(size_t)r * m + c] = T[(size_t)c * m + r] = next_entry();
    run_step("real", m, 1, which, T);
  }
  for (int m : orders) {
    std::vector<double> T((size_t)2 * m * m);
    for (int r = 0; r < m; ++r)
      for (int c = r; c < m; ++c) {
        const double re = next_entry(), im = r == c ? 0.0 : next_entry();
        T[2 * ((size_t)r * m + c)] = T[2 * ((size_t)c * m + r)] = re;
        T[2 * ((size_t)r * m + c) + 1] = im;
        T[2 * ((size_t)c * m + r) + 1] = r == c ? 0.0 : -im;
      }
    run_step("hermitian", m, 2, which, T);
  }
  // equal values keep their places: two pairs with no coupling, one pair planted through a rotation, a pair of
  // opposite sign (equal in magnitude only)
  run_step("pairs", 4, 1, which, {2.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 1.0});
  run_step("planted", 3, 1, which, {2.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0});
  run_step("signs", 3, 1, which, {-1.5, 0.0, 0.0, 0.0, 0.25, 0.0, 0.0, 0.0, 1.5});
  run_step("nan", 2, 1, which, {1.0, NAN, NAN, 2.0});
  run_step("inf", 2, 1, which, {1.0, 0.5, 0.5, INFINITY});
  run_step("nan", 2, 2, which, {1.0, 0.0, 0.5, NAN, 0.5, NAN, 2.0, 0.0});
}

}  // namespace

int main() {
  const int orders[5] = {1, 2, 3, 17, 60};
  for (int m : orders) run_real(m);
  for (int m : orders) run_hermitian(m);
  // a coupling so small that both diagonals absorb it is dropped, not rotated
  double T[8] = {1.0, 0.0, 1e-30, 1e-30, 1e-30, -1e-30, 2.0, 0.0}, Y[8];
  const int sweeps = spl::ritz_jacobi_hermitian(2, T, Y);
  expect(sweeps == 1 && T[0] == 1.0 && T[6] == 2.0 && T[2] == 0.0 && T[3] == 0.0 && Y[0] == 1.0 && Y[6] == 1.0,
         "a negligible coupling", 2);
  for (int which = 0; which < 3; ++which) run_steps(which);
  std::printf("bad %d\n", bad);
  return bad == 0 ? 0 : 1;
}

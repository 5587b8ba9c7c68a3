// ritz_jacobi.hpp — the Ritz step of the two eigensolvers (eigsh.hip: thick-restart Lanczos; lobpcg.hip: LOBPCG): cyclic
// Jacobi on the projected matrix, real symmetric and complex Hermitian, and the order of the values, in plain C++ on the
// host: no device code, no library type.  The rules are written out in include/sparse_linear_hip.h (the real one in
// the Lanczos section, the complex one in the LOBPCG section); a product and a sum are rounded apart
// (-ffp-contract=off).  tests/native/ritz_jacobi_check.cpp runs all of it under the sanitizers.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>

namespace spl {

constexpr int kRitzMaxSweeps = 60;

// T: m x m real symmetric, full storage, T[r * m + c]; Y: m x m, receives the vectors as columns (Y = I at the start).
// T's diagonal becomes the values.  Sweeps started, or -1 past kRitzMaxSweeps
inline int ritz_jacobi_real(int m, double *T, double *Y) {
  auto at = [m](double *M, int r, int c) -> double & { return M[(size_t)r * m + c]; };
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < m; ++c) at(Y, r, c) = r == c ? 1.0 : 0.0;
  for (int sweeps = 0;; ++sweeps) {
    bool any = false;
    for (int p = 0; p < m && !any; ++p)
      for (int q = p + 1; q < m; ++q)
        if (at(T, p, q) != 0.0) { any = true; break; }
    if (!any) return sweeps;
    if (sweeps == kRitzMaxSweeps) return -1;
    for (int p = 0; p < m; ++p)
      for (int q = p + 1; q < m; ++q) {
        const double a = at(T, p, q);
        if (a == 0.0) continue;
        const double app = at(T, p, p), aqq = at(T, q, q);
        if (std::fabs(app) + std::fabs(a) == std::fabs(app) && std::fabs(aqq) + std::fabs(a) == std::fabs(aqq)) {
          at(T, p, q) = at(T, q, p) = 0.0;
          continue;
        }
        const double tau = (aqq - app) / (2.0 * a);
        const double den = std::fabs(tau) + std::sqrt(1.0 + tau * tau);
        const double tt = (tau >= 0.0 ? 1.0 : -1.0) / den;
        const double c = 1.0 / std::sqrt(1.0 + tt * tt), s = tt * c;
        for (int r = 0; r < m; ++r) {
          if (r == p || r == q) continue;
          const double rp = at(T, r, p), rq = at(T, r, q);
          const double np = c * rp - s * rq, nq = s * rp + c * rq;
          at(T, r, p) = at(T, p, r) = np;
          at(T, r, q) = at(T, q, r) = nq;
        }
        at(T, p, p) = app - tt * a;
        at(T, q, q) = aqq + tt * a;
        at(T, p, q) = at(T, q, p) = 0.0;
        for (int r = 0; r < m; ++r) {
          const double rp = at(Y, r, p), rq = at(Y, r, q);
          at(Y, r, p) = c * rp - s * rq;
          at(Y, r, q) = s * rp + c * rq;
        }
      }
  }
}

// T: m x m complex Hermitian, full storage as packed pairs, entry (r, c) at T[2 * (r * m + c)], the diagonal real
// (its imaginary parts are not read and are left alone); Y likewise, Y = I at the start.  The rule of the real one
// with the coupling a = T_pq turned real first: g = |a|, u = a / g, column q times conj(u), then the real rotation
// from g.  Sweeps started, or -1 past kRitzMaxSweeps
inline int ritz_jacobi_hermitian(int m, double *T, double *Y) {
  auto re = [m](double *M, int r, int c) -> double & { return M[2 * ((size_t)r * m + c)]; };
  auto im = [m](double *M, int r, int c) -> double & { return M[2 * ((size_t)r * m + c) + 1]; };
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < m; ++c) {
      re(Y, r, c) = r == c ? 1.0 : 0.0;
      im(Y, r, c) = 0.0;
    }
  for (int sweeps = 0;; ++sweeps) {
    bool any = false;
    for (int p = 0; p < m && !any; ++p)
      for (int q = p + 1; q < m; ++q)
        if (re(T, p, q) != 0.0 || im(T, p, q) != 0.0) { any = true; break; }
    if (!any) return sweeps;
    if (sweeps == kRitzMaxSweeps) return -1;
    for (int p = 0; p < m; ++p)
      for (int q = p + 1; q < m; ++q) {
        const double ar = re(T, p, q), ai = im(T, p, q);
        if (ar == 0.0 && ai == 0.0) continue;
        const double g = std::sqrt(ar * ar + ai * ai);
        const double app = re(T, p, p), aqq = re(T, q, q);
        if (std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) {
          re(T, p, q) = re(T, q, p) = 0.0;
          im(T, p, q) = im(T, q, p) = 0.0;
          continue;
        }
        const double ur = ar / g, ui = ai / g;  // the phase; column q is multiplied by its conjugate (ur, -ui)
        const double tau = (aqq - app) / (2.0 * g);
        const double den = std::fabs(tau) + std::sqrt(1.0 + tau * tau);
        const double tt = (tau >= 0.0 ? 1.0 : -1.0) / den;
        const double c = 1.0 / std::sqrt(1.0 + tt * tt), s = tt * c;
        // (x, y) (ur, -ui) = (x ur + y ui, y ur - x ui): Data.Complex's product with b = -ui, so "- b d" is "+ y ui"
        for (int r = 0; r < m; ++r) {
          if (r == p || r == q) continue;
          const double pr = re(T, r, p), pi = im(T, r, p), xr = re(T, r, q), xi = im(T, r, q);
          const double qr = xr * ur + xi * ui, qi = xi * ur - xr * ui;
          const double npr = c * pr - s * qr, npi = c * pi - s * qi;
          const double nqr = s * pr + c * qr, nqi = s * pi + c * qi;
          re(T, r, p) = npr;
          im(T, r, p) = npi;
          re(T, p, r) = npr;
          im(T, p, r) = -npi;
          re(T, r, q) = nqr;
          im(T, r, q) = nqi;
          re(T, q, r) = nqr;
          im(T, q, r) = -nqi;
        }
        re(T, p, p) = app - tt * g;
        re(T, q, q) = aqq + tt * g;
        re(T, p, q) = re(T, q, p) = 0.0;
        im(T, p, q) = im(T, q, p) = 0.0;
        for (int r = 0; r < m; ++r) {
          const double pr = re(Y, r, p), pi = im(Y, r, p), xr = re(Y, r, q), xi = im(Y, r, q);
          const double qr = xr * ur + xi * ui, qi = xi * ur - xr * ui;
          re(Y, r, p) = c * pr - s * qr;
          im(Y, r, p) = c * pi - s * qi;
          re(Y, r, q) = s * pr + c * qr;
          im(Y, r, q) = s * pi + c * qi;
        }
      }
  }
}

// What a close does with its projected matrix: the rule (width 1: ritz_jacobi_real; 2: ritz_jacobi_hermitian, T and Y
// in that rule's layout), then `order`: the m indices stable-sorted by the values T_ii after `which`, one of the
// SPL_EIGSH_* orders (0 largest first, 1 smallest first, 2 largest magnitude first).  Sweeps started; -1 when the rule
// does not converge or a value or an entry of Y is not finite (order is not written then)
inline int ritz_step(int m, int width, int which, double *T, double *Y, int *order) {
  const int sweeps = width == 1 ? ritz_jacobi_real(m, T, Y) : ritz_jacobi_hermitian(m, T, Y);
  if (sweeps < 0) return -1;
  auto value = [&](int i) { return T[((size_t)i * m + i) * width]; };
  for (int i = 0; i < m; ++i)
    if (!std::isfinite(value(i))) return -1;
  for (size_t q = 0; q < (size_t)m * m * width; ++q)
    if (!std::isfinite(Y[q])) return -1;
  for (int i = 0; i < m; ++i) order[i] = i;
  std::stable_sort(order, order + m, [&](int a, int b) {
    if (which == 0) return value(a) > value(b);
    if (which == 1) return value(a) < value(b);
    return std::fabs(value(a)) > std::fabs(value(b));
  });
  return sweeps;
}

}  // namespace spl

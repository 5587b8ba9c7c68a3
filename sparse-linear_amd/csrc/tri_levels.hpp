// tri_levels.hpp — host tables of the sparse triangular solve (trisolve.hip): the triangle of every CSR row, the level
// number of every row, the rows bucketed by level and the launch plan that cuts the levels into segments.  Plain C++17,
// no HIP: tests/native/tri_levels_check.cpp restates every table from the pattern alone and compares.
//
// The pattern handed to levels() and plan() is the OFF-DIAGONAL part of the triangle in original row order: row i
// holds the columns j it waits for, all below i (lower) or all above i (upper), ascending.
//   level(i) = 1 + max level(j) over those columns, 0 for a row that has none.
// A lower triangle is in topological order when i ascends, an upper one when i descends, so one pass computes the
// levels.  Rows are bucketed by level with i ascending inside a level; position p in that order is the row's place in
// the permuted image the kernels read.
//
// Launch plan.  A level of at least `small_rows` rows is WIDE: one launch of the row-groups frame, a group of G lanes
// per row, G from the mean row length of the level.  A run of consecutive levels that are each below `small_rows` is
// NARROW: one launch of a single workgroup that walks the levels with a workgroup barrier between them; a narrow
// segment holds at most `segment_levels` levels, so no kernel's running time is unbounded.  Dependencies are kept by
// launch order on the stream and by that barrier, by nothing else.
#pragma once

#include <stdint.h>
#include <stdlib.h>
#include <vector>

namespace spl {
namespace tri {

// Defaults (measured: profiles/trisolve_bench.json).  64 rows: a narrow level is walked by ONE
// workgroup of 256 threads, which takes 64 rows of 4 lanes each in one pass; a level of one pass costs about 0.5 us there
// (a chain of dependent loads) against 2.7 to 4.8 us for a launch of its own, and from a few passes on the launch wins.
// 1024 levels: a segment then stays well below a millisecond per 1000 levels, the launches it saves are all but the
// last 2 % of what there is to save, and a bidiagonal matrix of 10^6 rows is about a thousand launches, not a million.
constexpr int kSmallRowsDefault = 64;
constexpr int kSegmentLevelsDefault = 1024;
constexpr int kSmallRowsMax = 1 << 30;
constexpr int kSegmentLevelsMax = 1 << 16;

struct Knobs {
  int small_rows = kSmallRowsDefault;          // SPL_TRSV_SMALL_ROWS, 1 ... 2^30: 1 makes every level wide
  int segment_levels = kSegmentLevelsDefault;  // SPL_TRSV_SEGMENT_LEVELS, 1 ... 65536
};

inline int clamp_knob(long long v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : (int)v; }

// the one reader of the two environment variables; called once per analysis.  Unset, empty or not a number: the default
inline Knobs read_knobs() {
  Knobs k;
  auto read = [](const char *name, int dflt, int lo, int hi) {
    const char *s = getenv(name);
    if (!s || !*s) return dflt;
    char *end = nullptr;
    const long long v = strtoll(s, &end, 10);
    if (end == s) return dflt;
    return clamp_knob(v, lo, hi);
  };
  k.small_rows = read("SPL_TRSV_SMALL_ROWS", kSmallRowsDefault, 1, kSmallRowsMax);
  k.segment_levels = read("SPL_TRSV_SEGMENT_LEVELS", kSegmentLevelsDefault, 1, kSegmentLevelsMax);
  return k;
}

// smallest power of two >= mean, 1 ... 64 (group_for of row_groups.hpp, restated for the host-only header)
inline int group_for_mean(double mean) {
  int g = 1;
  while (g < 64 && (double)g < mean) g <<= 1;
  return g;
}

// entries of the ascending run j[a .. b) that are < x (count_less of row_groups.hpp on the host)
inline int count_less(const int *j, int64_t a, int64_t b, int x) {
  int64_t lo = a, hi = b;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (j[mid] < x) lo = mid + 1; else hi = mid;
  }
  return (int)(lo - a);
}

// The triangle of a square CSR pattern whose rows ascend strictly.  Row i of the result holds the off-diagonal run of
// the triangle: off_ptr (n + 1), off_col, off_src (position of the entry in the source arrays); diag_src[i] is the
// position of the stored a_ii or -1.  *stored = entries of the triangle, stored diagonals included; *longest = the
// longest row of it, counted the same way.
struct Triangle {
  std::vector<int> off_ptr, off_col, off_src, diag_src;
  int64_t stored = 0, longest = 0;
};

inline void take_triangle(int n, const int *rowptr, const int *colidx, bool lower, Triangle &T) {
  T.off_ptr.assign((size_t)n + 1, 0);
  T.diag_src.assign((size_t)n, -1);
  T.stored = 0;
  T.longest = 0;
  std::vector<int> first((size_t)n);
  for (int i = 0; i < n; ++i) {
    const int s = rowptr[i], e = rowptr[i + 1];
    const int below = count_less(colidx, s, e, i);  // entries with j < i
    const bool has_diag = s + below < e && colidx[s + below] == i;
    if (has_diag) T.diag_src[i] = s + below;
    const int len = lower ? below : (e - s) - below - (has_diag ? 1 : 0);
    first[i] = lower ? s : e - len;
    T.off_ptr[i + 1] = T.off_ptr[i] + len;
    const int64_t with_diag = (int64_t)len + (has_diag ? 1 : 0);
    T.stored += with_diag;
    if (with_diag > T.longest) T.longest = with_diag;
  }
  const size_t nnz = (size_t)T.off_ptr[n];
  T.off_col.resize(nnz);
  T.off_src.resize(nnz);
  for (int i = 0; i < n; ++i) {
    const int o = T.off_ptr[i], len = T.off_ptr[i + 1] - o;
    for (int e = 0; e < len; ++e) {
      T.off_col[o + e] = colidx[first[i] + e];
      T.off_src[o + e] = first[i] + e;
    }
  }
}

// level[i] for an off-diagonal pattern in original row order; returns the number of levels (0 for n == 0)
inline int levels(int n, const int *ptr, const int *col, bool lower, std::vector<int> &level) {
  level.assign((size_t)n, 0);
  int top = -1;
  for (int t = 0; t < n; ++t) {
    const int i = lower ? t : n - 1 - t;
    int l = 0;
    for (int q = ptr[i]; q < ptr[i + 1]; ++q) {
      const int lj = level[col[q]] + 1;
      if (lj > l) l = lj;
    }
    level[i] = l;
    if (l > top) top = l;
  }
  return top + 1;
}

enum SegmentKind { kWide = 0, kNarrow = 1 };

struct Segment {
  int kind;            // kWide: one level; kNarrow: levels [level0, level1) walked by one workgroup
  int level0, level1;
  int row0, row1;      // positions in the permuted order: level_ptr[level0], level_ptr[level1]
  int group;           // lanes per row
};

struct Plan {
  int nlevels = 0;
  std::vector<int> level_ptr;  // nlevels + 1: first position of every level
  std::vector<int> rows;       // n: original row at every position, ascending inside a level
  std::vector<int> pos;        // n: position of every original row
  std::vector<Segment> segments;
  int64_t launches() const { return (int64_t)segments.size(); }  // kernels one solve of one column group enqueues
};

inline void plan(int n, const int *ptr, const std::vector<int> &level, int nlevels, const Knobs &knobs, Plan &P) {
  P.nlevels = nlevels;
  P.level_ptr.assign((size_t)nlevels + 1, 0);
  P.rows.assign((size_t)n, 0);
  P.pos.assign((size_t)n, 0);
  P.segments.clear();
  for (int i = 0; i < n; ++i) P.level_ptr[(size_t)level[i] + 1]++;
  for (int l = 0; l < nlevels; ++l) P.level_ptr[l + 1] += P.level_ptr[l];
  std::vector<int> next(P.level_ptr.begin(), P.level_ptr.end() - (nlevels > 0 ? 1 : 0));
  for (int i = 0; i < n; ++i) {  // ascending i: ascending inside every level
    const int p = next[level[i]]++;
    P.rows[p] = i;
    P.pos[i] = p;
  }
  // entries of every level, for the mean row length
  std::vector<int64_t> entries((size_t)nlevels, 0);
  for (int i = 0; i < n; ++i) entries[level[i]] += ptr[i + 1] - ptr[i];
  auto mean_group = [](int64_t e, int rows) { return group_for_mean(rows > 0 ? (double)e / (double)rows : 0.0); };
  int l = 0;
  while (l < nlevels) {
    const int rows_l = P.level_ptr[l + 1] - P.level_ptr[l];
    if (rows_l >= knobs.small_rows) {
      P.segments.push_back(Segment{kWide, l, l + 1, P.level_ptr[l], P.level_ptr[l + 1], mean_group(entries[l], rows_l)});
      ++l;
      continue;
    }
    int m = l;
    int64_t e = 0;
    while (m < nlevels && m - l < knobs.segment_levels && P.level_ptr[m + 1] - P.level_ptr[m] < knobs.small_rows) {
      e += entries[m];
      ++m;
    }
    P.segments.push_back(Segment{kNarrow, l, m, P.level_ptr[l], P.level_ptr[m], mean_group(e, P.level_ptr[m] - P.level_ptr[l])});
    l = m;
  }
}

// The permuted image of an off-diagonal pattern: row p of the result is original row P.rows[p]
inline void permute_rows(int n, const int *ptr, const int *col, const int *src, const Plan &P, std::vector<int> &pptr,
                         std::vector<int> &pcol, std::vector<int> &psrc) {
  pptr.assign((size_t)n + 1, 0);
  for (int p = 0; p < n; ++p) pptr[p + 1] = pptr[p] + (ptr[P.rows[p] + 1] - ptr[P.rows[p]]);
  pcol.resize((size_t)pptr[n]);
  psrc.resize((size_t)pptr[n]);
  for (int p = 0; p < n; ++p) {
    const int i = P.rows[p], o = pptr[p];
    for (int e = 0; e < ptr[i + 1] - ptr[i]; ++e) {
      pcol[o + e] = col[ptr[i] + e];
      psrc[o + e] = src[ptr[i] + e];
    }
  }
}

// The order-preserving transpose of a permuted image (pptr / pcol over positions, P its plan): row j of the result
// holds the original rows i that have an entry in column j, ascending, and tsrc the position of that entry in the
// permuted arrays.  A lower triangle becomes an upper one and the reverse.
inline void transpose_image(int n, const std::vector<int> &pptr, const std::vector<int> &pcol, const Plan &P,
                            std::vector<int> &tptr, std::vector<int> &tcol, std::vector<int> &tsrc) {
  tptr.assign((size_t)n + 1, 0);
  for (size_t q = 0; q < pcol.size(); ++q) tptr[(size_t)pcol[q] + 1]++;
  for (int j = 0; j < n; ++j) tptr[j + 1] += tptr[j];
  tcol.resize(pcol.size());
  tsrc.resize(pcol.size());
  std::vector<int> next(tptr.begin(), tptr.end() - 1 + (n == 0 ? 1 : 0));
  for (int i = 0; i < n; ++i) {  // ascending original row: ascending inside every new row
    const int p = P.pos[i];
    for (int q = pptr[p]; q < pptr[p + 1]; ++q) {
      const int o = next[pcol[q]]++;
      tcol[o] = i;
      tsrc[o] = q;
    }
  }
}

}  // namespace tri
}  // namespace spl

// mf_levels.hpp — host tables of the multifrontal LU (multifrontal.hip): the size limits and switches of a
// factorisation, its transient memory plan, and — per tree level — which fronts go to which kernel and the prefix
// sums that turn a level into flat grids, for the factorisation and the solves alike.  Integer arithmetic on the tree
// of mf_symbolic.hpp only.  Plain C++17, no HIP: compiled into the library and into the CPU self-check
// tests/native/levels_check.cpp, which restates every table from the tree alone.
#pragma once

#include <stdint.h>
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "mf_symbolic.hpp"

namespace spl {

// ---- the constants the tables (and the kernels that read them) depend on
constexpr int NB = 64;              // panel width of the dense kernels (dense_lu_kernels.hpp)
constexpr int SB = 4;               // blocks of NB pivots a super-block step of the blocked solves eliminates
constexpr int kSmallFront = 128;    // fronts up to this size are factored by one workgroup each
constexpr int kMidFront = 4096;     // ... up to this size in lockstep with the others of their level
// fronts above this size are solved by many workgroups, in lockstep (round 5: 256 -> 128 — with the pivot blocks as chains of
// matrix-vector products the many-workgroup path is the faster one for all but the leaves: 100^3 11.4 -> 10.3 ms per solve,
// 64^3 4.9 -> 4.1, 40^3 2.45 -> 2.06, complex 100^3 18.6 -> 17.6; 64 gives the same)
constexpr int kBigSolve = 128;
constexpr int kSolveRowBlocks = 4;  // blocks of 64 rows per workgroup in the lockstep solve steps
constexpr int kGemvChunk = 512;     // boundary columns per workgroup of the chunked boundary products
constexpr int kTileCols = 16;       // a workgroup moves 64 rows x 16 columns: 4 columns per thread

namespace mf {

// The switches of a numeric factorisation, read from the environment once per mf_factor call.
struct FactorKnobs {
  int small_limit = kSmallFront;  // SPL_MF_SMALL (at least 64)
  // medium fronts (small_limit < size <= mid_limit) go through the lockstep kernels: SPL_MF_MIDMAX; SPL_MF_MID=0
  // sends them down the per-front pipeline instead (ablation: mid_limit = small_limit)
  int mid_limit = kMidFront;
  int big_solve = kBigSolve;      // SPL_MF_BIGSOLVE (at least 64)
  bool mid_paired = true;         // SPL_MF_MIDPAIR=0: K = 64 every step (ablation)
  bool overlap = true;            // SPL_MF_OVERLAP=0: assembly on the main stream
  int forced_cut = -1;            // SPL_MF_CUT (tests: force a cut depth; the user clamps it to the tree's depth); -1: none
  bool timing = false;            // SPL_MF_TIMING: phase times on stderr (diagnostic)
};

inline FactorKnobs read_factor_knobs() {
  auto value = [](const char *name, int unset) {
    const char *e = getenv(name);
    return e ? atoi(e) : unset;
  };
  FactorKnobs k;
  k.small_limit = std::max(64, value("SPL_MF_SMALL", kSmallFront));
  k.big_solve = std::max(64, value("SPL_MF_BIGSOLVE", kBigSolve));
  k.mid_limit = value("SPL_MF_MID", 1) == 0 ? k.small_limit : std::max(value("SPL_MF_MIDMAX", kMidFront), k.small_limit);
  k.mid_paired = value("SPL_MF_MIDPAIR", 1) != 0;
  k.overlap = value("SPL_MF_OVERLAP", 1) != 0;
  k.forced_cut = getenv("SPL_MF_CUT") ? std::max(0, value("SPL_MF_CUT", 0)) : -1;
  k.timing = getenv("SPL_MF_TIMING") != nullptr;
  return k;
}

// doubles of one plane of the whole front f (TreeView::fplane is the device's copy of this)
inline int64_t front_elems(const Tree &T, int f) {
  return ((int64_t)T.ld[(size_t)f] * std::max(T.fs(f), 1) + 15) / 16 * 16;
}

// ---- transient memory plan of the numeric factorisation.  With cut = 0 the tree is processed level by
// level as a whole: the whole fronts of a level and of its children are alive together.  With
// cut = K > 0 the subtrees hanging below depth K are processed one after the other (each needs
// only its own share of every level), the Schur complement of each subtree root waits in the
// `cut` buffer, and the top K levels come last.  The smallest K that fits the budget is used.
struct Plan {
  int cut = 0;
  std::vector<int64_t> foff;         // offset of every whole front inside its region (per segment and level)
  std::vector<int64_t> cboff;        // offset of the saved Schur complement of a subtree root, or -1
  std::vector<int> first;            // smallest id of the subtree of every front
  std::vector<int> roots;            // the fronts at depth `cut` (ascending ids); empty for cut = 0
  int64_t region_elems[2] = {0, 0}, cut_elems = 0;
  int64_t transient_elems() const { return region_elems[0] + region_elems[1] + cut_elems; }
};

inline Plan make_plan(const Tree &T, int cut) {
  Plan P;
  P.cut = cut;
  const int nf = T.nfronts, nd = T.maxdepth + 1;
  P.foff.assign((size_t)nf, 0);
  P.cboff.assign((size_t)nf, -1);
  P.first.resize((size_t)nf);
  for (int f = 0; f < nf; ++f) P.first[(size_t)f] = f;
  for (int f = 0; f < nf; ++f)
    if (T.parent[(size_t)f] >= 0)
      P.first[(size_t)T.parent[(size_t)f]] = std::min(P.first[(size_t)T.parent[(size_t)f]], P.first[(size_t)f]);
  // lays out the fronts with ids in [lo, hi] and depths in [dtop, dend): returns nothing, grows the regions
  auto layout = [&](int lo, int hi, int dtop, int dend) {
    for (int d = dtop; d < dend; ++d) {
      const std::vector<int> &L = T.by_depth[(size_t)d];
      int64_t off = 0;
      for (auto it = std::lower_bound(L.begin(), L.end(), lo); it != L.end() && *it <= hi; ++it) {
        P.foff[(size_t)*it] = off;
        off += front_elems(T, *it);
      }
      P.region_elems[d & 1] = std::max(P.region_elems[d & 1], off);
    }
  };
  if (cut <= 0 || cut >= nd) {
    P.cut = 0;
    layout(0, nf - 1, 0, nd);
    return P;
  }
  P.roots = T.by_depth[(size_t)cut];
  for (int r : P.roots) {
    layout(P.first[(size_t)r], r, cut, nd);
    P.cboff[(size_t)r] = P.cut_elems;
    P.cut_elems += ((int64_t)T.nb[(size_t)r] * T.nb[(size_t)r] + 15) / 16 * 16;
  }
  layout(0, nf - 1, 0, cut);  // the top: depths < cut (their lists hold nothing else)
  return P;
}

// ---- the fronts of one depth that are solved by many workgroups, and the flat grids of their lockstep solve
// kernels: segments of count + 1 prefix sums (workgroups, or doubles, before each front), one per Grid (and step)
struct BigLevel {
  enum class Grid {
    // one segment per super-block step k in [0, steps)
    fwd,         // forward steps over all fs rows of a front (untransposed, SPL_MF_SPLIT_FWD=0)
    fwd_t,       // forward steps over the np pivot rows (transposed systems; untransposed with the boundary split off)
    bwd,         // backward steps over the pivot block
    // one segment each
    boundary_t,        // boundary kernel of the transposed forward pass: 4 boundary columns per workgroup
    gather,            // 256 boundary rows per workgroup; what is left of it: total > 0 = some front has a boundary
    gemv,              // backward boundary product (np rows x nb columns) in chunks of kGemvChunk columns
    gemv_reduce,       // ... the reduction of its chunks (fronts with more than one)
    gemv_offsets,      // ... offsets of the fronts in its scratch (doubles per right-hand-side column)
    fwd_gemv,          // the same three for the forward boundary product (nb rows x np columns)
    fwd_gemv_reduce,
    fwd_gemv_offsets,
    // one segment per launch k in [0, steps]: lead groups of step k + bulk groups of step k - 1
    pipe_fwd,    // pipelined forward pass over the pivot block
    pipe_bwd     // pipelined backward pass
  };
  static constexpr int kStepGrids = 3, kSingleGrids = 8, kPipeGrids = 2;

  int count = 0, steps = 0;
  int row_blocks = 1;  // blocks of 64 rows per workgroup in the super-block steps (levels that fill the chip: more)
  std::vector<int> list;
  std::vector<int64_t> h;

  size_t segments() const { return (size_t)kStepGrids * steps + kSingleGrids + (size_t)kPipeGrids * (steps + 1); }
  size_t seg(Grid grid, int k = 0) const {  // where the segment starts in h (and in its device copy)
    const size_t g = (size_t)grid, pipe0 = (size_t)Grid::pipe_fwd;
    size_t which;
    if (g < (size_t)kStepGrids) which = g * (size_t)steps + (size_t)k;
    else if (g < pipe0) which = (size_t)kStepGrids * steps + (g - kStepGrids);
    else which = (size_t)kStepGrids * steps + kSingleGrids + (g - pipe0) * (size_t)(steps + 1) + (size_t)k;
    return which * (size_t)(count + 1);
  }
  int64_t sum(Grid grid, int k = 0) const { return h[seg(grid, k) + (size_t)count]; }
  unsigned total(Grid grid, int k = 0) const { return (unsigned)sum(grid, k); }
  const int64_t *prefix(Grid grid, int k = 0) const { return h.data() + seg(grid, k); }
};

inline BigLevel build_big_level(const Tree &T, std::vector<int> large) {
  using Grid = BigLevel::Grid;
  BigLevel B;
  B.count = (int)large.size();
  if (B.count == 0) return B;
  constexpr int span = SB * NB;
  auto np_of = [&](int f) { return T.np[(size_t)f]; };
  auto nb_of = [&](int f) { return T.nb[(size_t)f]; };
  for (int f : large) B.steps = std::max(B.steps, (np_of(f) + span - 1) / span);
  // every workgroup of a step redoes the in-super-block solve: where the first step alone
  // would launch thousands of workgroups, each takes kSolveRowBlocks blocks of rows instead
  int64_t first_step = 0;
  for (int f : large) first_step += (T.fs(f) + 63) / 64;
  B.row_blocks = first_step >= 4096 ? kSolveRowBlocks : 1;
  const int rbk = B.row_blocks;
  B.list = std::move(large);
  B.h.assign(B.segments() * (size_t)(B.count + 1), 0);
  auto fill = [&](Grid grid, int k, auto groups_of) {
    int64_t *pre = B.h.data() + B.seg(grid, k);
    for (int i = 0; i < B.count; ++i) pre[i + 1] = pre[i] + groups_of(B.list[(size_t)i]);
  };
  for (int k = 0; k < B.steps; ++k) {
    auto fwd_rows = [&](int f, int n) -> int64_t {  // workgroups of forward step k of a pass over n rows
      const int np = np_of(f), j0 = k * span;
      if (j0 >= np) return 0;
      const int jbs = std::min(span, np - j0);
      return std::max(1, ((n - (j0 + jbs) + 63) / 64 + rbk - 1) / rbk);
    };
    fill(Grid::fwd, k, [&](int f) { return fwd_rows(f, T.fs(f)); });
    fill(Grid::fwd_t, k, [&](int f) { return fwd_rows(f, np_of(f)); });
    fill(Grid::bwd, k, [&](int f) -> int64_t {
      const int nsup = (np_of(f) + span - 1) / span;
      if (k >= nsup) return 0;
      return std::max(1, (((nsup - 1 - k) * span + 63) / 64 + rbk - 1) / rbk);
    });
  }
  for (int k = 0; k <= B.steps; ++k) {
    auto groups = [&](int f, bool forward) -> int64_t {
      const int np = np_of(f), nsup = (np + span - 1) / span;
      auto beyond = [&](int st) {  // rows of the pivot block still to be updated by step st
        const int j0 = (forward ? st : nsup - 1 - st) * span, jbs = std::min(span, np - j0);
        return forward ? np - (j0 + jbs) : j0;
      };
      int64_t g = 0;
      if (k < nsup) g += std::max(1, std::min(SB, (beyond(k) + 63) / 64));
      if (k >= 1 && k - 1 < nsup) {
        const int rest = beyond(k - 1) - span;
        if (rest > 0) g += ((rest + 63) / 64 + rbk - 1) / rbk;
      }
      return g;
    };
    fill(Grid::pipe_fwd, k, [&](int f) { return groups(f, true); });
    fill(Grid::pipe_bwd, k, [&](int f) { return groups(f, false); });
  }
  fill(Grid::boundary_t, 0, [&](int f) -> int64_t { return (nb_of(f) + 3) / 4; });
  fill(Grid::gather, 0, [&](int f) -> int64_t { return (nb_of(f) + 255) / 256; });
  auto chunks = [&](int f) -> int64_t { return (nb_of(f) + kGemvChunk - 1) / kGemvChunk; };
  fill(Grid::gemv, 0, [&](int f) -> int64_t { return (int64_t)((np_of(f) + 63) / 64) * chunks(f); });
  fill(Grid::gemv_reduce, 0, [&](int f) -> int64_t { return chunks(f) > 1 ? (np_of(f) + 255) / 256 : 0; });
  fill(Grid::gemv_offsets, 0, [&](int f) -> int64_t { return chunks(f) > 1 ? chunks(f) * np_of(f) : 0; });
  auto fchunks = [&](int f) -> int64_t { return (np_of(f) + kGemvChunk - 1) / kGemvChunk; };
  fill(Grid::fwd_gemv, 0, [&](int f) -> int64_t { return (int64_t)((nb_of(f) + (np_of(f) & 15) + 63) / 64) * fchunks(f); });
  fill(Grid::fwd_gemv_reduce, 0, [&](int f) -> int64_t { return fchunks(f) > 1 ? (nb_of(f) + 255) / 256 : 0; });
  fill(Grid::fwd_gemv_offsets, 0, [&](int f) -> int64_t { return fchunks(f) > 1 ? fchunks(f) * nb_of(f) : 0; });
  return B;
}

// ---- the lockstep medium fronts of a level and the prefix arrays of their block steps:
// [step][phase 0 = panel solves, 1 = update][count + 1]
struct Mid {
  int count = 0, steps = 0;  // steps: block steps of the longest front
  std::vector<int> list;
  std::vector<int64_t> h;
  size_t seg(int step, int phase) const { return ((size_t)step * 2 + (size_t)phase) * (size_t)(count + 1); }
  int64_t sum(int step, int phase) const { return h[seg(step, phase) + (size_t)count]; }
};

// the medium fronts among the fronts [b0, b1) of a level's list (the whole level, or a subtree's share of a cut tree)
inline Mid mid_fronts(const Tree &T, const std::vector<int> &fronts, int b0, int b1, const FactorKnobs &knobs) {
  Mid M;
  for (int i = b0; i < b1; ++i) {
    const int f = fronts[(size_t)i];
    if (T.np[(size_t)f] == 0 || T.fs(f) <= knobs.small_limit || T.fs(f) > knobs.mid_limit) continue;
    M.list.push_back(f);
    M.steps = std::max(M.steps, (T.np[(size_t)f] + NB - 1) / NB);
  }
  M.count = (int)M.list.size();
  M.h.assign((size_t)M.steps * 2 * (size_t)(M.count + 1), 0);
  for (int st = 0; st < M.steps; ++st) {
    int64_t *pt = M.h.data() + M.seg(st, 0), *pu = M.h.data() + M.seg(st, 1);
    for (int k = 0; k < M.count; ++k) {
      const int f = M.list[(size_t)k], np = T.np[(size_t)f], j0 = st * NB;
      int64_t tt = 0, tu = 0;
      if (j0 < np) {
        const int jb = std::min(NB, np - j0), rest = T.fs(f) - (j0 + jb);
        const int64_t nt = (rest + 63) / 64;
        tt = 2 * nt;
        tu = nt * nt;
        if (knobs.mid_paired && !(st & 1) && np >= j0 + jb + NB) tu = 2 * nt - 1;  // (the L-shaped pass of an even step)
      }
      pt[k + 1] = pt[k] + tt;
      pu[k + 1] = pu[k] + tu;
    }
  }
  return M;
}

// ---- everything about the levels that depends on the tree and the size limits only: built by the first
// factorisation of a tree on a device and shared by all that follow.  The fronts of depth d are T.by_depth[d]; every
// list below is a subsequence of such a list (ascending ids).
struct LevelTables {
  int small_limit = 0, mid_limit = 0, big_solve = 0;  // what they were built for
  bool mid_paired = true;
  bool built_for(const FactorKnobs &k) const {
    return small_limit == k.small_limit && mid_limit == k.mid_limit && big_solve == k.big_solve && mid_paired == k.mid_paired;
  }
  struct Level {
    std::vector<int> small;     // fronts factored by one workgroup each
    std::vector<int> solve;     // fronts solved by one workgroup each
    std::vector<int> child[2];  // children (by slot) of the fronts of this depth
    int child_maxnb[2] = {0, 0};  // ... and the largest boundary among them
    // the flat grids of compaction, assembly and extend-add: tiles (64 x kTileCols) before each front of the level
    // (P and U panels), groups of 32 pivots (atile), tiles before each item of child[] (Schur complements)
    std::vector<int64_t> ptile, utile, atile, ctile[2];
    BigLevel big;  // fronts solved by many workgroups (those above big_solve that have pivots)
    Mid mid;       // the medium fronts of the whole level
  };
  std::vector<Level> levels;
  int64_t gemv_scratch = 0;  // doubles per right-hand-side column the chunked boundary products of a level need at most
};

inline LevelTables build_level_tables(const Tree &T, const FactorKnobs &knobs) {
  using Grid = BigLevel::Grid;
  LevelTables L;
  L.small_limit = knobs.small_limit;
  L.mid_limit = knobs.mid_limit;
  L.big_solve = knobs.big_solve;
  L.mid_paired = knobs.mid_paired;
  const int nd = T.maxdepth + 1;
  L.levels.resize((size_t)nd);
  auto tiles = [](int64_t rows, int64_t cols) { return ((rows + 63) / 64) * ((cols + kTileCols - 1) / kTileCols); };
  for (int d = 0; d < nd; ++d) {
    const std::vector<int> &fronts = T.by_depth[(size_t)d];
    LevelTables::Level &V = L.levels[(size_t)d];
    std::vector<int> large;
    V.ptile.assign(1, 0);
    V.utile.assign(1, 0);
    V.atile.assign(1, 0);
    for (int f : fronts) {
      const int np = T.np[(size_t)f], nb = T.nb[(size_t)f];
      if (np > 0 && T.fs(f) <= knobs.small_limit) V.small.push_back(f);
      if (T.fs(f) <= knobs.big_solve) V.solve.push_back(f);
      else if (np > 0) large.push_back(f);
      V.ptile.push_back(V.ptile.back() + tiles(T.fs(f), np));
      V.utile.push_back(V.utile.back() + tiles(np, nb));
      V.atile.push_back(V.atile.back() + (np + 31) / 32);
    }
    V.big = build_big_level(T, std::move(large));
    if (V.big.count > 0)
      L.gemv_scratch = std::max({L.gemv_scratch, V.big.sum(Grid::gemv_offsets), V.big.sum(Grid::fwd_gemv_offsets)});
    if (d + 1 < nd)
      for (int c : T.by_depth[(size_t)d + 1]) V.child[T.slot[(size_t)c]].push_back(c);
    for (int sl = 0; sl < 2; ++sl) {
      V.ctile[sl].assign(1, 0);
      for (int c : V.child[sl]) {
        V.child_maxnb[sl] = std::max(V.child_maxnb[sl], T.nb[(size_t)c]);
        V.ctile[sl].push_back(V.ctile[sl].back() + tiles(T.nb[(size_t)c], T.nb[(size_t)c]));
      }
    }
    V.mid = mid_fronts(T, fronts, 0, (int)fronts.size(), knobs);
  }
  return L;
}

}  // namespace mf
}  // namespace spl

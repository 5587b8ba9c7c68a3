// CPU self-check of the level tables of the multifrontal LU (sparse-linear_amd/csrc/mf_levels.hpp): reads "n nnz" then
// Ap (n+1) and Ai (nnz) from stdin, builds the tree (mf_symbolic.hpp), the tables (build_level_tables, with the SPL_MF_*
// switches of the environment) and the memory plans (make_plan), and checks every list and prefix array against a
// restatement from the tree alone: the closed forms below are written out with literal tile sizes, not taken from the
// header.  Prints one line of key=value statistics; exit status 0 iff nothing is wrong.
//   argv[1]: leaf size of the dissection (256); argv[2]: 1 = the tables must exercise every class (a level with small,
//   medium and many-workgroup fronts at once, large fronts, a level of more than one super-block step)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mf_levels.hpp"

using namespace spl::mf;
using Grid = BigLevel::Grid;

static long bad = 0;
#define CHECK(cond) \
  do { \
    if (!(cond)) { \
      if (++bad <= 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
    } \
  } while (0)

static int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static int64_t tiles(int64_t rows, int64_t cols) { return cdiv(rows, 64) * cdiv(cols, 16); }

// `pre` holds count + 1 prefix sums whose steps are item(i)
template <typename F>
static void check_prefix(const int64_t *pre, size_t count, F item) {
  CHECK(pre[0] == 0);
  int64_t sum = 0;
  for (size_t i = 0; i < count; ++i) {
    CHECK(pre[i + 1] >= pre[i]);
    sum += item(i);
    CHECK(pre[i + 1] == sum);
  }
}

static bool ascending(const std::vector<int> &v) {
  for (size_t i = 1; i < v.size(); ++i)
    if (v[i - 1] >= v[i]) return false;
  return true;
}

// workgroups of block step `st` of a medium front: panel solves (phase 0) and update (phase 1)
static int64_t mid_groups(int np, int fs, int st, int phase, bool paired) {
  const int done0 = 64 * st;
  if (done0 >= np) return 0;
  const int done1 = done0 + 64 < np ? done0 + 64 : np;  // pivots eliminated after this step
  const int64_t nt = cdiv(fs - done1, 64);              // blocks of rows (and of columns) behind the pivot block
  if (phase == 0) return 2 * nt;                        // the L and the U panel
  // an even step with a whole pivot block behind it updates only the L-shaped border; the odd step does both (K = 128)
  if (paired && st % 2 == 0 && np - done1 >= 64) return 2 * nt - 1;
  return nt * nt;
}

// workgroups of super-block step k (256 pivots) of a forward pass over n rows, rbk blocks of 64 rows each
static int64_t fwd_groups(int np, int n, int k, int rbk) {
  if (256 * k >= np) return 0;
  const int done = 256 * (k + 1) < np ? 256 * (k + 1) : np;
  const int64_t g = cdiv(cdiv(n - done, 64), rbk);
  return g > 0 ? g : 1;
}
static int64_t bwd_groups(int np, int k, int rbk) {
  const int nsup = (int)cdiv(np, 256);
  if (k >= nsup) return 0;
  const int64_t g = cdiv(4 * (int64_t)(nsup - 1 - k), rbk);  // the rows above super block nsup - 1 - k, in blocks of 64
  return g > 0 ? g : 1;
}
// launch k of a pipelined pass: the lead groups of step k (at most 4, the blocks next to the super block) and the bulk
// groups of step k - 1 (the rows further than one super block away)
static int64_t pipe_groups(int np, int k, int rbk, bool forward) {
  const int nsup = (int)cdiv(np, 256);
  auto left = [&](int st) -> int64_t {  // rows of the pivot block not yet solved after step st
    if (!forward) return 256 * (int64_t)(nsup - 1 - st);
    return np - (256 * (int64_t)(st + 1) < np ? 256 * (int64_t)(st + 1) : np);
  };
  int64_t g = 0;
  if (k < nsup) {
    int64_t lead = cdiv(left(k), 64);
    if (lead > 4) lead = 4;
    if (lead < 1) lead = 1;
    g += lead;
  }
  if (k >= 1 && k <= nsup && left(k - 1) > 256) g += cdiv(cdiv(left(k - 1) - 256, 64), rbk);
  return g;
}

// 3. the grids of the many-workgroup solves of the fronts B.list, 4. with the scratch their chunked products need
struct BigStats {
  int steps = 0, row_blocks = 0;
  int64_t scratch = 0;
};
static BigStats check_big_level(const Tree &T, const BigLevel &B) {
  const std::vector<int> &big = B.list;
  auto NP = [&](int f) { return T.np[(size_t)f]; };
  auto NBD = [&](int f) { return T.nb[(size_t)f]; };
  auto FS = [&](int f) { return T.np[(size_t)f] + T.nb[(size_t)f]; };
  BigStats out;
  CHECK(B.count == (int)big.size());
  if (big.empty()) {
    CHECK(B.h.empty() && B.steps == 0);
    return out;
  }
  int steps = 0;
  int64_t blocks = 0;
  for (int f : big) {
    steps = steps > (int)cdiv(NP(f), 256) ? steps : (int)cdiv(NP(f), 256);
    blocks += cdiv(FS(f), 64);
  }
  const int rbk = blocks >= 4096 ? 4 : 1;  // a first step of thousands of workgroups: four blocks of rows each
  CHECK(B.steps == steps && B.row_blocks == rbk);
  out.steps = steps;
  out.row_blocks = rbk;
  // 3 grids per step, 8 single ones, 2 per launch of a pipelined pass; no two segments overlap
  const size_t nseg = (size_t)3 * steps + 8 + (size_t)2 * (steps + 1);
  CHECK(B.segments() == nseg && B.h.size() == nseg * (big.size() + 1));
  if (!(B.steps == steps && B.h.size() == nseg * (big.size() + 1))) return out;
  std::vector<char> taken(nseg, 0);
  auto grid = [&](Grid g, int k, auto item) {
    const size_t at = B.seg(g, k);
    CHECK(at % (big.size() + 1) == 0 && at / (big.size() + 1) < nseg);
    if (at % (big.size() + 1) != 0 || at / (big.size() + 1) >= nseg) return;
    CHECK(!taken[at / (big.size() + 1)]);
    taken[at / (big.size() + 1)] = 1;
    CHECK(B.prefix(g, k) == B.h.data() + at);
    check_prefix(B.h.data() + at, big.size(), [&](size_t i) { return (int64_t)item(big[i]); });
    CHECK(B.sum(g, k) == B.h[at + big.size()] && B.total(g, k) == (unsigned)B.h[at + big.size()]);
  };
  for (int k = 0; k < steps; ++k) {
    grid(Grid::fwd, k, [&](int f) { return fwd_groups(NP(f), FS(f), k, rbk); });
    grid(Grid::fwd_t, k, [&](int f) { return fwd_groups(NP(f), NP(f), k, rbk); });
    grid(Grid::bwd, k, [&](int f) { return bwd_groups(NP(f), k, rbk); });
  }
  for (int k = 0; k <= steps; ++k) {
    grid(Grid::pipe_fwd, k, [&](int f) { return pipe_groups(NP(f), k, rbk, true); });
    grid(Grid::pipe_bwd, k, [&](int f) { return pipe_groups(NP(f), k, rbk, false); });
  }
  grid(Grid::boundary_t, 0, [&](int f) { return cdiv(NBD(f), 4); });
  grid(Grid::gather, 0, [&](int f) { return cdiv(NBD(f), 256); });
  // backward boundary product: np rows in blocks of 64, nb columns in chunks of 512; more than one chunk: partial
  // sums in scratch (chunks x np doubles per column) and a reduction over the np rows
  grid(Grid::gemv, 0, [&](int f) { return cdiv(NP(f), 64) * cdiv(NBD(f), 512); });
  grid(Grid::gemv_reduce, 0, [&](int f) { return NBD(f) > 512 ? cdiv(NP(f), 256) : 0; });
  grid(Grid::gemv_offsets, 0, [&](int f) { return NBD(f) > 512 ? cdiv(NBD(f), 512) * NP(f) : 0; });
  // forward: nb rows, and np mod 16 masked ones before them so that every block starts on a whole line; np columns
  grid(Grid::fwd_gemv, 0, [&](int f) { return cdiv(NBD(f) + NP(f) % 16, 64) * cdiv(NP(f), 512); });
  grid(Grid::fwd_gemv_reduce, 0, [&](int f) { return NP(f) > 512 ? cdiv(NBD(f), 256) : 0; });
  grid(Grid::fwd_gemv_offsets, 0, [&](int f) { return NP(f) > 512 ? cdiv(NP(f), 512) * NBD(f) : 0; });
  for (char t : taken) CHECK(t);
  int64_t back = 0, fwd = 0;
  for (int f : big) {
    if (NBD(f) > 512) back += cdiv(NBD(f), 512) * NP(f);
    if (NP(f) > 512) fwd += cdiv(NP(f), 512) * NBD(f);
  }
  out.scratch = back > fwd ? back : fwd;
  return out;
}

// A level that fills the chip — 4096 blocks of 64 rows and more among its many-workgroup fronts, 262 144 rows: no grid a
// test can dissect in seconds has one — from front sizes written down by hand: row_blocks = 4 in every step grid.
static void check_wide_level() {
  Tree T;
  std::vector<int> fronts;
  for (int f = 0; f < 120; ++f) {
    T.np.push_back(f % 7 == 0 ? 0 : 190 * (f % 9) + 3 * f + 1);  // 7 super blocks and more, some fronts without pivots
    T.nb.push_back(2500 + 37 * (f % 5) - 2400 * (f % 11 == 0));
    if (T.np.back() > 0) fronts.push_back(f);
  }
  T.nfronts = 120;
  const BigStats st = check_big_level(T, build_big_level(T, fronts));
  CHECK(st.row_blocks == 4 && st.steps >= 7 && st.scratch > 0);
}

int main(int argc, char **argv) {
  const int leaf = argc > 1 ? atoi(argv[1]) : 256;
  const bool require_all = argc > 2 && atoi(argv[2]) != 0;
  int n = 0, nnz = 0;
  if (scanf("%d %d", &n, &nnz) != 2) return 2;
  std::vector<int> Ap((size_t)n + 1), Ai((size_t)nnz);
  for (int &v : Ap) if (scanf("%d", &v) != 1) return 2;
  for (int &v : Ai) if (scanf("%d", &v) != 1) return 2;
  Tree T;
  build_tree(n, Ap.data(), Ai.data(), leaf, T);
  const FactorKnobs K = read_factor_knobs();
  const LevelTables L = build_level_tables(T, K);
  const int nd = T.maxdepth + 1, nf = T.nfronts;
  auto NP = [&](int f) { return T.np[(size_t)f]; };
  auto NBD = [&](int f) { return T.nb[(size_t)f]; };
  auto FS = [&](int f) { return T.np[(size_t)f] + T.nb[(size_t)f]; };

  CHECK(L.built_for(K) && (int)L.levels.size() == nd);
  CHECK(K.small_limit >= 64 && K.big_solve >= 64 && K.mid_limit >= K.small_limit);
  long n_small = 0, n_mid = 0, n_large = 0, n_big = 0, multi_step = 0, all_three = 0, max_rbk = 0;
  int64_t scratch = 0;
  for (int d = 0; d < nd; ++d) {
    const std::vector<int> &fronts = T.by_depth[(size_t)d];
    const LevelTables::Level &V = L.levels[(size_t)d];
    // 1. the classes of the factorisation and of the solves partition the level
    std::vector<int> small, mid, solve, big;
    long large = 0;
    for (int f : fronts) {
      CHECK(T.depth[(size_t)f] == d);
      if (NP(f) > 0) {
        if (FS(f) <= K.small_limit) small.push_back(f);
        else if (FS(f) <= K.mid_limit) mid.push_back(f);
        else ++large;
      }
      if (FS(f) <= K.big_solve) solve.push_back(f);
      else if (NP(f) > 0) big.push_back(f);
    }
    CHECK(ascending(fronts));
    CHECK(V.small == small && V.mid.list == mid && V.solve == solve && V.big.list == big);
    CHECK(V.mid.count == (int)mid.size() && V.big.count == (int)big.size());
    n_small += (long)small.size();
    n_mid += (long)mid.size();
    n_large += large;
    n_big += (long)big.size();
    if (!small.empty() && !mid.empty() && !big.empty()) ++all_three;
    // 2. the children, by slot
    std::vector<int> child[2];
    int maxnb[2] = {0, 0};
    if (d + 1 < nd)
      for (int c : T.by_depth[(size_t)d + 1]) {
        const int sl = T.slot[(size_t)c];
        CHECK(sl == 0 || sl == 1);
        CHECK(T.parent[(size_t)c] >= 0 && T.depth[(size_t)T.parent[(size_t)c]] == d);
        child[sl & 1].push_back(c);
        if (NBD(c) > maxnb[sl & 1]) maxnb[sl & 1] = NBD(c);
      }
    for (int sl = 0; sl < 2; ++sl) {
      CHECK(V.child[sl] == child[sl] && V.child_maxnb[sl] == maxnb[sl]);
      // 3. tile prefixes of the Schur complements
      CHECK(V.ctile[sl].size() == child[sl].size() + 1);
      if (V.ctile[sl].size() == child[sl].size() + 1)
        check_prefix(V.ctile[sl].data(), child[sl].size(), [&](size_t i) { return tiles(NBD(child[sl][i]), NBD(child[sl][i])); });
    }
    // 3. tile prefixes of the panels and of the assembly
    CHECK(V.ptile.size() == fronts.size() + 1 && V.utile.size() == fronts.size() + 1 && V.atile.size() == fronts.size() + 1);
    if (V.ptile.size() == fronts.size() + 1 && V.utile.size() == fronts.size() + 1 && V.atile.size() == fronts.size() + 1) {
      check_prefix(V.ptile.data(), fronts.size(), [&](size_t i) { return tiles(FS(fronts[i]), NP(fronts[i])); });
      check_prefix(V.utile.data(), fronts.size(), [&](size_t i) { return tiles(NP(fronts[i]), NBD(fronts[i])); });
      check_prefix(V.atile.data(), fronts.size(), [&](size_t i) { return cdiv(NP(fronts[i]), 32); });
    }
    // 3. the medium fronts: panel solves and update of every block step
    {
      const Mid &M = V.mid;
      int steps = 0;
      for (int f : mid) steps = steps > (int)cdiv(NP(f), 64) ? steps : (int)cdiv(NP(f), 64);
      CHECK(M.steps == steps);
      CHECK(M.h.size() == (size_t)steps * 2 * (mid.size() + 1));
      if (M.steps == steps && M.h.size() == (size_t)steps * 2 * (mid.size() + 1) && M.list == mid)
        for (int st = 0; st < steps; ++st)
          for (int phase = 0; phase < 2; ++phase) {
            const int64_t *pre = M.h.data() + ((size_t)st * 2 + (size_t)phase) * (mid.size() + 1);
            check_prefix(pre, mid.size(), [&](size_t i) { return mid_groups(NP(mid[i]), FS(mid[i]), st, phase, K.mid_paired); });
            CHECK(M.sum(st, phase) == pre[mid.size()]);
          }
    }
    // 3. the grids of the many-workgroup solves, 4. the scratch of their chunked products
    CHECK(V.big.list == big);
    if (V.big.list == big) {
      const BigStats st = check_big_level(T, V.big);
      if (st.steps > 1) ++multi_step;
      if (st.row_blocks > max_rbk) max_rbk = st.row_blocks;
      if (st.scratch > scratch) scratch = st.scratch;
    }
    // 5. the medium fronts of a part of the level (a subtree of a cut tree) are those of the whole level in that part
    for (int part = 0; part < 3 && fronts.size() >= 3; ++part) {
      const int b0 = (int)(fronts.size() * part / 3), b1 = (int)(fronts.size() * (part + 1) / 3);
      const Mid S = mid_fronts(T, fronts, b0, b1, K);
      std::vector<int> want;
      for (int f : mid)
        if (f >= fronts[(size_t)b0] && f <= fronts[(size_t)b1 - 1]) want.push_back(f);
      CHECK(S.list == want && S.count == (int)want.size());
      int steps = 0;
      for (int f : want) steps = steps > (int)cdiv(NP(f), 64) ? steps : (int)cdiv(NP(f), 64);
      CHECK(S.steps == steps && S.h.size() == (size_t)steps * 2 * (want.size() + 1));
      if (S.list != want || S.steps != steps || S.h.size() != (size_t)steps * 2 * (want.size() + 1) || want.empty()) continue;
      // ... with the whole level's prefix steps: where `want` starts in the level's list
      size_t first = 0;
      while (V.mid.list[first] != want[0]) ++first;
      for (int st = 0; st < steps; ++st)
        for (int phase = 0; phase < 2; ++phase) {
          const int64_t *whole = V.mid.h.data() + V.mid.seg(st, phase) + first, *sub = S.h.data() + S.seg(st, phase);
          for (size_t i = 0; i <= want.size(); ++i) CHECK(sub[i] == whole[i] - whole[0]);
        }
    }
  }
  CHECK(L.gemv_scratch == scratch);
  check_wide_level();

  // 6. the memory plans: whole tree, cut depths inside the tree, a cut beyond it
  long plans = 0;
  for (int cut : {0, 1, 2, nd - 1, nd, nd + 7}) {
    if (cut < 0) continue;
    const Plan P = make_plan(T, cut);
    const int eff = (cut <= 0 || cut >= nd) ? 0 : cut;
    CHECK(P.cut == eff);
    CHECK((int)P.foff.size() == nf && (int)P.cboff.size() == nf && (int)P.first.size() == nf);
    if ((int)P.foff.size() != nf || (int)P.cboff.size() != nf || (int)P.first.size() != nf) continue;
    ++plans;
    // first: the smallest id below every front (post-order: a subtree is the id range [first, f])
    std::vector<int> first((size_t)nf);
    for (int f = 0; f < nf; ++f) first[(size_t)f] = f;
    for (int f = 0; f < nf; ++f) {
      const int p = T.parent[(size_t)f];
      if (p >= 0 && first[(size_t)f] < first[(size_t)p]) first[(size_t)p] = first[(size_t)f];
    }
    CHECK(P.first == first);
    CHECK(eff == 0 ? P.roots.empty() : P.roots == T.by_depth[(size_t)eff]);
    // segment of a front: the subtree root above it at the cut depth (-1: the top of the tree, or no cut)
    std::vector<int> segment((size_t)nf, -1);
    if (eff > 0)
      for (int f = nf - 1; f >= 0; --f) {
        if (T.depth[(size_t)f] == eff) segment[(size_t)f] = f;
        else if (T.depth[(size_t)f] > eff) segment[(size_t)f] = segment[(size_t)T.parent[(size_t)f]];
      }
    int64_t cut_elems = 0;
    for (int f = 0; f < nf; ++f) {
      if (eff > 0 && T.depth[(size_t)f] == eff) {
        CHECK(P.cboff[(size_t)f] == cut_elems);
        cut_elems += cdiv((int64_t)NBD(f) * NBD(f), 16) * 16;
      } else {
        CHECK(P.cboff[(size_t)f] == -1);
      }
    }
    CHECK(P.cut_elems == cut_elems);
    CHECK(P.transient_elems() == P.region_elems[0] + P.region_elems[1] + cut_elems);
    // fronts of one level and one segment follow each other without overlap, inside the level's region
    for (int d = 0; d < nd; ++d) {
      const std::vector<int> &fronts = T.by_depth[(size_t)d];
      int64_t end = 0;
      int seg = -2;
      for (int f : fronts) {
        const int fs = FS(f) > 1 ? FS(f) : 1;
        const int64_t elems = cdiv((int64_t)T.ld[(size_t)f] * fs, 16) * 16;
        CHECK(front_elems(T, f) == elems && T.ld[(size_t)f] >= FS(f));
        if (segment[(size_t)f] != seg) {  // (ids of a segment are contiguous in a level's ascending list)
          seg = segment[(size_t)f];
          end = 0;
        }
        CHECK(P.foff[(size_t)f] >= end && P.foff[(size_t)f] % 16 == 0);
        end = P.foff[(size_t)f] + elems;
        CHECK(end <= P.region_elems[d & 1]);
      }
    }
  }

  if (require_all) CHECK(all_three > 0 && n_large > 0 && multi_step > 0);
  printf("n=%d fronts=%d depth=%d small=%ld mid=%ld large=%ld big=%ld all_three_levels=%ld multi_step_levels=%ld "
         "row_blocks=%ld gemv_scratch=%lld plans=%ld small_limit=%d mid_limit=%d big_solve=%d mid_paired=%d overlap=%d "
         "forced_cut=%d timing=%d bad=%ld\n",
         n, nf, T.maxdepth, n_small, n_mid, n_large, n_big, all_three, multi_step, max_rbk, (long long)L.gemv_scratch,
         plans, K.small_limit, K.mid_limit, K.big_solve, (int)K.mid_paired, (int)K.overlap, K.forced_cut, (int)K.timing, bad);
  return bad != 0;
}

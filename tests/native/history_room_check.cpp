// CPU self-check of the growth rule of a solve's device history (sparse-linear_amd/csrc/history_room.hpp) with a stub
// store: a host array that is reallocated to exactly the size asked for, so that a write past the capacity is a heap
// overflow the address sanitizer sees.  It replays the calls CG / BiCGSTAB (krylov.hip) and GMRES (gmres.hip) make,
// writes what a batch writes, and compares every capacity with the rule as it stood before the two copies were folded,
// written out below as a plain function.  Prints one line of key=value statistics; exit status 0 iff nothing is wrong.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "history_room.hpp"

static long bad = 0;
#define CHECK(cond) \
  do { \
    if (!(cond)) { \
      if (++bad <= 20) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
    } \
  } while (0)

struct StubStore {
  double *p = nullptr;
  long long n = 0;
  long grows = 0;
  bool wanted() const { return true; }
  long long capacity() const { return n; }
  void grow(long long want, long long written) {
    double *bigger = static_cast<double *>(malloc((size_t)want * sizeof(double)));
    if (written > 0) memcpy(bigger, p, (size_t)written * sizeof(double));
    free(p);
    p = bigger;
    n = want;
    ++grows;
  }
  ~StubStore() { free(p); }
};

struct Unwanted {
  bool wanted() const { return false; }
  long long capacity() const { return 0; }
  void grow(long long, long long) { ++bad; }
};

// The rule of the parent commit (GRun::room_for; Run::room_for was the same without the first line, and every caller
// of it passed entries <= max_iter + 1): the capacity after the call
static long long parent_capacity(long long have, long long entries, long long max_iter) {
  if (entries > max_iter + 1) entries = max_iter + 1;
  if (have < entries) {
    long long want = 2 * have > entries ? 2 * have : entries;
    if (want < 64) want = 64;
    if (want > max_iter + 1) want = max_iter + 1;
    return want;
  }
  return have;
}

// one call, checked: the parent's capacity, never above max_iter + 1 unless it was there before, what was written kept
static void call(StubStore &store, long long entries, long long written, long long max_iter) {
  const long long before = store.capacity(), expect = parent_capacity(before, entries, max_iter);
  spl::room_for(store, entries, written, max_iter);
  CHECK(store.capacity() == expect);
  CHECK(store.capacity() <= (before > max_iter + 1 ? before : max_iter + 1));
  for (long long i = 0; i < written; ++i) CHECK(store.p[i] == (double)i);
}

// CG and BiCGSTAB: room for the batch before its first iteration; iteration `it` writes history[it]
static long krylov(StubStore &store, long long max_iter, int every, long long converge_at) {
  long calls = 0;
  auto batch_end = [&](long long issued) { return issued + every < max_iter ? issued + every : max_iter; };
  call(store, batch_end(0) + 1, 0, max_iter), ++calls;
  store.p[0] = 0.0;  // the start writes history[0]
  for (long long issued = 0; issued < max_iter;) {
    if (issued % every == 0) {
      call(store, batch_end(issued) + 1, issued + 1, max_iter), ++calls;
      CHECK(store.capacity() >= batch_end(issued) + 1);  // what the batch writes
    }
    ++issued;
    store.p[issued] = (double)issued;
    if ((issued % every == 0 || issued == max_iter) && issued >= converge_at) break;
  }
  return calls;
}

// GMRES: `every` cycles of up to m iterations between two looks; a cycle may close early (here: after `per_cycle`)
static long gmres(StubStore &store, long long max_iter, long long every, int m, int per_cycle, long long converge_at) {
  long calls = 0;
  call(store, every * m + 1, 0, max_iter), ++calls;
  store.p[0] = 0.0;
  long long it = 0;
  for (long long issued = 0;;) {
    for (int j = 0; j < m && j < per_cycle && it < max_iter; ++j) {  // the device stops a cycle at max_iter
      ++it;
      store.p[it] = (double)it;
    }
    ++issued;
    if (issued % every == 0) {
      if (it >= converge_at || it >= max_iter) break;
      call(store, it + every * m + 1, it + 1, max_iter), ++calls;
      const long long next = it + every * m < max_iter ? it + every * m : max_iter;
      CHECK(store.capacity() >= next + 1);  // what the cycles up to the next look write at most
    }
  }
  return calls;
}

int main() {
  const long long max_iters[] = {0, 1, 63, 64, 65, 1000};
  const int everys[] = {1, 16, 100};
  const int restarts[] = {1, 5, 128};
  long calls = 0, grows = 0, runs = 0;
  for (long long max_iter : max_iters) {
    for (int every : everys) {
      for (long long converge_at : {max_iter, max_iter / 2, (long long)1}) {
        {
          StubStore store;
          calls += krylov(store, max_iter, every, converge_at);
          // a second solve on the same object finds the store as the first left it
          calls += krylov(store, max_iter / 2, every, max_iter / 2);
          grows += store.grows, ++runs;
        }
        for (int m : restarts)
          for (int per_cycle : {m, (m + 1) / 2}) {
            StubStore store;
            calls += gmres(store, max_iter, every, m, per_cycle, converge_at);
            calls += gmres(store, max_iter / 2, every, m, per_cycle, max_iter / 2);
            grows += store.grows, ++runs;
          }
      }
    }
  }
  Unwanted none;
  spl::room_for(none, 100, 0, 1000);  // no history: nothing is allocated
  // the clamp itself: a caller that asks for more than a solve can write gets max_iter + 1
  {
    StubStore store;
    call(store, 1000, 0, 9);
    CHECK(store.capacity() == 10);
    for (int i = 0; i < 10; ++i) store.p[i] = (double)i;
    call(store, 1000, 10, 200);
    CHECK(store.capacity() == 201);
  }
  printf("bad=%ld runs=%ld calls=%ld grows=%ld\n", bad, runs, calls, grows);
  return bad == 0 ? 0 : 1;
}

// history_room.hpp — how the device history of an iterative solve grows (CG, BiCGSTAB and GMRES: solver_core.hpp).
// Plain C++ over a store, so that the rule is checked on the CPU with a stub store (tests/native/history_room_check.cpp).
#pragma once

namespace spl {

// Room for `entries` values of the history, of which `written` may be written already; no solve writes more than
// max_iter + 1.  The store grows with the iterations that were issued, in steps of what the caller asks for at least
// and by doubling, never with max_iter.  Store: wanted() (false: the caller keeps no history), capacity(), and
// grow(want, written), which keeps the first `written`.
template <typename Store>
void room_for(Store &store, long long entries, long long written, long long max_iter) {
  if (!store.wanted()) return;
  if (entries > max_iter + 1) entries = max_iter + 1;
  const long long have = store.capacity();
  if (have >= entries) return;
  long long want = 2 * have > entries ? 2 * have : entries;
  if (want < 64) want = 64;
  if (want > max_iter + 1) want = max_iter + 1;
  store.grow(want, written);
}

}  // namespace spl

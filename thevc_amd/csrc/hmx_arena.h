// Placement in the argument arena: a ring of `cap` bytes in which the host tables of a call (unit lists, prefix sums, picture
// tables) are put at 256-byte steps.  Pure host arithmetic, no HIP: arena_reserve / arena_place / arena_push (hmx_core.hip) do the
// copies and the stream synchronisation around it, tests/native/arena_host.cpp runs it on the CPU.
//
// A call first reserves the sum of the rounded sizes of ALL the tables it will put before its kernel is launched, then places
// them one by one:
//   reserve(total)  kRefused when total > cap (head unchanged: nothing was placed, nothing may be copied or launched);
//                   kWrap when the tables do not fit behind head: head is 0 again, and the caller must wait for everything
//                   issued so far before it copies -- tables of EARLIER calls may still be read by their kernels;
//                   kStay otherwise.
//   place(bytes)    the offset of the next table, or kNone when the table is not covered by what the call reserved.
// So a call wraps at most once, in front of its first table; its tables are disjoint and inside [0, cap); and a table is never
// put over another table of the same call, whose kernel has not been launched yet -- no wait could make that safe.
#pragma once
#include <cstddef>

struct ArenaCursor {
  static constexpr size_t kAlign = 256, kNone = ~(size_t)0;
  enum Reserve { kRefused = -1, kStay = 0, kWrap = 1 };
  size_t cap = 0, head = 0;
  size_t open = 0; // bytes of the current reservation that are not placed yet: head + open <= cap

  static constexpr size_t rounded(size_t bytes) { return (bytes + kAlign - 1) & ~(kAlign - 1); }

  Reserve reserve(size_t total_of_rounded_sizes) {
    open = 0; // what an earlier call reserved and did not place is gone
    if (total_of_rounded_sizes > cap) return kRefused;
    open = total_of_rounded_sizes;
    if (head + open > cap) {
      head = 0;
      return kWrap;
    }
    return kStay;
  }
  size_t place(size_t bytes) {
    const size_t r = rounded(bytes);
    if (r > open) return kNone; // serving it could only wrap onto the call's own tables
    const size_t at = head;
    head += r, open -= r;
    return at;
  }
};

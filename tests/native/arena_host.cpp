// The placement rule of the argument arena (thevc_amd/csrc/hmx_arena.h) on the CPU, beside a model of the rule it replaced, for
// tests/test_arena_placement.py.  No GPU and no HIP: only the arithmetic that decides where a call's tables go.
//
// stdin, one scenario per line:   cap head  k r s1 .. sk  [k r s1 .. sk ...]
//   a ring of `cap` bytes whose head stands at `head`, then calls in order; a call puts k tables of s1 .. sk bytes before its
//   launch and reserves the first r of them (r = k is what the library does; r < k shows what happens to a table outside the
//   reservation).
// stdout, one line per scenario, per call:
//   N status head k off1 .. offk     the new rule: status -1 refused / 0 placed behind head / 1 wrapped in front of the first table,
//                                    head after the call, the offsets (-1: not placed)
//   O head k off1 .. offk            the old rule: every push on its own, wrapping whenever it does not fit (-1: larger than cap)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "hmx_arena.h"

namespace {
// the rule before reserve-then-place: a table that does not fit behind head goes to offset 0, whatever lies there
struct OldRing {
  size_t cap, head;
  long long push(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes > cap) return -1;
    if (head + bytes > cap) head = 0;
    const size_t at = head;
    head += bytes;
    return (long long)at;
  }
};
} // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    size_t cap, head;
    if (!(in >> cap >> head)) continue;
    ArenaCursor cur;
    cur.cap = cap, cur.head = head;
    OldRing old{cap, head};
    std::ostringstream out;
    size_t k, r;
    while (in >> k >> r) {
      std::vector<size_t> s(k);
      for (size_t &v : s)
        if (!(in >> v)) return 2;
      size_t total = 0;
      for (size_t i = 0; i < r && i < k; i++) total += ArenaCursor::rounded(s[i]);
      const int status = (int)cur.reserve(total);
      std::vector<long long> at(k, -1);
      if (status != ArenaCursor::kRefused)
        for (size_t i = 0; i < k; i++) {
          const size_t p = cur.place(s[i]);
          at[i] = p == ArenaCursor::kNone ? -1 : (long long)p;
        }
      out << "N " << status << ' ' << cur.head << ' ' << k;
      for (long long v : at) out << ' ' << v;
      out << " O ";
      std::vector<long long> oat(k);
      for (size_t i = 0; i < k; i++) oat[i] = old.push(s[i]);
      out << old.head << ' ' << k;
      for (long long v : oat) out << ' ' << v;
      out << ' ';
    }
    std::puts(out.str().c_str());
  }
  return 0;
}

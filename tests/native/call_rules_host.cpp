// The host rules of a whole-picture call (thevc_amd/csrc/hmx_call_rules.h) on the CPU, for tests/test_call_rules.py.  No GPU and no
// HIP: the library's own header, asked one question per line.
//
// stdin, one query per line; stdout, one answer line per query:
//   E B q log2n                          rdoq_err_scale: the 64-bit pattern of the double, hexadecimal
//   F inv_scale per B lambda             rdoq_rd_factor; lambda as the 64-bit pattern of the double, hexadecimal
//   L q per B log2n                      rdoq_levels_fit16: 0 / 1
//   G knob_group rdoq n_pics             pack_group_rule
//   S n_pics I knob4 knob8 rdoq qmap max_levels sz0 sz1 sz2 sz3 items
//                                        pack_shape: n_groups n_shards slots4 slots8 n_rows waves_bound too_large
//   W knob_waves resident waves_bound max_levels
//                                        pack_wave_count
//   R resident plan_stride n_pics onto schedule across streams pipeline_conv graph
//                                        resolve_schedule: schedule across groups pipeline_conv
//   P s slots4 slots8                    pack_slots
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "hmx_call_rules.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    char op = 0;
    if (!(in >> op)) continue;
    if (op == 'E') {
      int B, q, lg;
      in >> B >> q >> lg;
      const double e = rdoq_err_scale(B, q, lg);
      uint64_t u;
      memcpy(&u, &e, 8);
      printf("%016" PRIx64 "\n", u);
    } else if (op == 'F') {
      int iq, per, B;
      uint64_t u;
      in >> iq >> per >> B >> std::hex >> u;
      double lam;
      memcpy(&lam, &u, 8);
      printf("%lld\n", rdoq_rd_factor(iq, per, lam, B));
    } else if (op == 'L') {
      int q, per, B, lg;
      in >> q >> per >> B >> lg;
      printf("%d\n", (int)rdoq_levels_fit16(q, per, B, lg));
    } else if (op == 'G') {
      int knob, rdoq, n;
      in >> knob >> rdoq >> n;
      printf("%d\n", pack_group_rule(knob, rdoq != 0, n));
    } else if (op == 'S') {
      int n, I, k4, k8, rdoq, qmap, levels;
      uint64_t sz[4], items;
      in >> n >> I >> k4 >> k8 >> rdoq >> qmap >> levels >> sz[0] >> sz[1] >> sz[2] >> sz[3] >> items;
      const PackShape r = pack_shape(n, I, k4, k8, rdoq != 0, qmap != 0, levels, sz, items);
      if (r.G.n_pics != n || r.G.I != I || r.G.max_levels != levels || r.items != items) return 3;
      printf("%d %d %d %d %" PRIu64 " %" PRIu64 " %d\n", r.G.n_groups, r.G.n_shards, r.G.slots4, r.G.slots8, r.n_rows, r.waves_bound, (int)r.too_large);
    } else if (op == 'W') {
      int knob, resident, max_levels;
      uint64_t bound;
      in >> knob >> resident >> bound >> max_levels;
      printf("%d\n", pack_wave_count(knob, resident, bound, max_levels));
    } else if (op == 'R') {
      struct {
        int schedule, across, streams;
        bool pipeline_conv, graph;
      } kn{};
      int resident, stride, n, onto, pipe, graph;
      in >> resident >> stride >> n >> onto >> kn.schedule >> kn.across >> kn.streams >> pipe >> graph;
      kn.pipeline_conv = pipe != 0, kn.graph = graph != 0;
      const CallSchedule s = resolve_schedule(resident != 0, stride, n, onto != 0, kn);
      printf("%d %d %d %d\n", s.schedule, (int)s.across, s.groups, (int)s.pipeline_conv);
    } else if (op == 'P') {
      int s, s4, s8;
      in >> s >> s4 >> s8;
      printf("%u\n", pack_slots(s, s4, s8));
    } else {
      return 2;
    }
    if (!in) return 2;
  }
  return 0;
}

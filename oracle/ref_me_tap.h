/* oracle/ref_me_tap.h -- TEST INFRASTRUCTURE (oracle/build_ref_enc_shim.sh, the TAppEncoder_metap build).  Force-included in
 * front of the reference's TEncSearch.cpp, whose xMotionEstimation, xTZSearchHelp and xPatternRefinement get recorder
 * statements between their own statements (oracle/ref_shim_edit.py TEncSearch metap); every statement of the reference stays
 * and runs as it is.  The recorder is idle unless the environment variable HMX_ME_TAP names a file; then each call of
 * xMotionEstimation appends to it
 *   the luma plane of its reference picture, margins included, the first time a reference POC is seen in the process:
 *     int32 {PIC_MAGIC, POC, width, height, margin x, margin y}; int16 plane[(height + 2 my) * (width + 2 mx)]
 *   and the call:
 *     int32 head[H_WORDS] (the H_* indices below); int16 org[h * w] (the pattern key's luma block as searched);
 *     int32 tz[3 * head[H_N_TZ]] = (iSearchX, iSearchY, cost after the vector term) of every xTZSearchHelp in order;
 *     uint32 frac[18] = the nine uiDist after the vector term of the half-sample, then of the quarter-sample xPatternRefinement
 * tests/golden/make_me_enc_tap.py samples such files into the fixture tests/golden/me_enc_tap.npz. */
#ifndef HMX_REF_ME_TAP_H
#define HMX_REF_ME_TAP_H
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>
enum {
  H_MAGIC, H_POC, H_LIST, H_REF_IDX, H_REF_POC, H_CU_X, H_CU_Y, H_X, H_Y, H_W, H_H, H_BI, H_FAST_SEARCH, H_FEN, H_HAD_ME, H_PRED_X, H_PRED_Y,
  H_MV_IN_X, H_MV_IN_Y, H_RANGE, H_ADAPT_RANGE, H_LAMBDA, H_BITS_IN, H_BITS_OUT, H_COST_OUT, H_LEFT, H_TOP, H_RIGHT, H_BOTTOM, H_INT_X, H_INT_Y,
  H_INT_SAD, H_HALF_X, H_HALF_Y, H_QTER_X, H_QTER_Y, H_FRAC_COST, H_MV_OUT_X, H_MV_OUT_Y, H_N_TZ, H_N_FRAC, H_BITS, H_PIC_W, H_PIC_H, H_CTU, H_WORDS
};
struct HmxMeTap {
  enum { PIC_MAGIC = 0x4d455049, CALL_MAGIC = 0x4d454341 };
  bool active;
  int head[H_WORDS];
  std::vector<short> org;
  std::vector<int> tz;
  unsigned frac[18];
  int n_frac;
  std::set<int> seen;
  HmxMeTap() : active(false), n_frac(0) {}
  static const char *path() { return getenv("HMX_ME_TAP"); }
  /* the reference picture's luma buffer WITH its margins: buf = the first sample of the top margin row */
  void picture(int poc, const short *buf, int w, int h, int mx, int my) {
    if (!path() || !seen.insert(poc).second) return;
    FILE *f = fopen(path(), "ab");
    if (!f) return;
    const int v[6] = {PIC_MAGIC, poc, w, h, mx, my};
    fwrite(v, sizeof(v), 1, f);
    fwrite(buf, sizeof(short), (size_t)(h + 2 * my) * (w + 2 * mx), f);
    fclose(f);
  }
  void begin(const short *blk, int stride, int w, int h) {
    active = path() != 0;
    if (!active) return;
    memset(head, 0, sizeof(head));
    memset(frac, 0, sizeof(frac));
    head[H_MAGIC] = CALL_MAGIC, head[H_W] = w, head[H_H] = h;
    n_frac = 0;
    tz.clear();
    org.resize((size_t)w * h);
    for (int r = 0; r < h; r++) memcpy(&org[(size_t)r * w], blk + (size_t)r * stride, sizeof(short) * w);
  }
  void set(int k, int v) {
    if (active) head[k] = v;
  }
  void tz_point(int x, int y, unsigned cost) {
    if (!active) return;
    tz.push_back(x), tz.push_back(y), tz.push_back((int)cost);
  }
  void frac_cost(unsigned cost) {
    if (!active) return;
    if (n_frac < 18) frac[n_frac] = cost;
    n_frac++;
  }
  void end() {
    if (!active) return;
    active = false;
    FILE *f = fopen(path(), "ab");
    if (!f) return;
    head[H_N_TZ] = (int)(tz.size() / 3), head[H_N_FRAC] = n_frac;
    fwrite(head, sizeof(head), 1, f);
    fwrite(org.data(), sizeof(short), org.size(), f);
    if (!tz.empty()) fwrite(tz.data(), sizeof(int), tz.size(), f);
    fwrite(frac, sizeof(frac), 1, f);
    fclose(f);
  }
};
static HmxMeTap g_hmx_me_tap;
#endif

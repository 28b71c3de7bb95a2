// hmx_chain_qmap.hip -- part of libhmx (include/hmx.h), gfx950.  See hmx_host.h for how the library is cut into translation units.
// The packed schedule's persistent kernel with a QP per block (hmx_set_qp_map): encoder with and without the distortion output, and
// decoder.  The quantiser constants are per-lane values here, which costs registers and instructions the single-QP kernel must not
// pay: these are instantiations of their own, in a translation unit of their own so that they compile beside the others.
#include "hmx_chain_dev.h"

int packed_qmap_max_blocks(int *nb) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(nb, k_intra_packed<true, 64, true, false, 8, true>, 64, 0) == hipSuccess ? 0 : -1;
}
void launch_packed_qmap(const PackArgsQ &A, bool enc, bool sse, unsigned n_wg, hipStream_t st) {
  const dim3 grid(n_wg), blk(64);
  if (!enc) hipLaunchKernelGGL((k_intra_packed<false, 64, false, false, 8, true>), grid, blk, 0, st, A);
  else if (sse) hipLaunchKernelGGL((k_intra_packed<true, 64, true, false, 8, true>), grid, blk, 0, st, A);
  else hipLaunchKernelGGL((k_intra_packed<true, 64, false, false, 8, true>), grid, blk, 0, st, A);
}

// The two largest instantiations of the register-resident LinearAttention backward (k_la_bwd.h): C >= 12 with 64-position rows (no
// BASELINE config uses them).  They crash this compiler's "AMDGPU Rewrite AGPR-Copy-MFMA" pass under -amdgpu-mfma-vgpr-form=1, so this
// translation unit is built without that option (the Makefile clears MFMA_FORM for its object in every build flavour).
#include "k_la_bwd.h"

namespace dq {

void launch_linattn_bwd_big(const LinAttnBwdK& kk, int C, int waves, hipStream_t s) {
  if (C == 12) hipLaunchKernelGGL((k_linattn_bwd<12, 64>), dim3(cdiv(waves, 4)), dim3(256), 0, s, kk);
  else hipLaunchKernelGGL((k_linattn_bwd<16, 64>), dim3(cdiv(waves, 4)), dim3(256), 0, s, kk);
}

}  // namespace dq

// "f32 via bf16x3" instantiations of the conv kernels (dpmn_set_compute_dtype(2); common.h x3_split2t, conv_body.h X3 paths):
// fp32 tensors in HBM, operands split exactly into three bf16 planes on the way into LDS, six v_mfma_f32_16x16x32_bf16 per
// product, fp32 accumulation and epilogues.  Same call sites as the fp32 kernels (cmm.py:38-77 convs, tsrn.py / tatt.py trunks):
// conv.hip routes a launch here when the mode is set and the variant exists.
#include "conv_body.h"

namespace {
template <int BM, int BN, int WM, int WN, bool AFF>
__global__ __launch_bounds__(256, 2) void k_conv_igemm_x3(ConvArgs a) {      // two resident blocks per CU, as the fp32 kernel
  conv_igemm_body<BM, BN, WM, WN, true, true, AFF, false, false, true>(a);
}
}  // namespace

namespace dpmn_conv {
int x3_launch_igemm(bool aff, const ConvArgs& a, dim3 grid, hipStream_t st) {
  if (aff) hipLaunchKernelGGL((k_conv_igemm_x3<128, 128, 2, 2, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_conv_igemm_x3<128, 128, 2, 2, false>), grid, dim3(256), 0, st, a);
  return 0;
}
int x3_launch_halo(const ConvArgs& a, dim3 grid, hipStream_t st) {
  constexpr int NPX = (8 + 2) * (16 + 2);
  const size_t smem = (size_t)(3 * NPX + 2 * 3 * 64) * ((BK + 8) / 2) * sizeof(float);
  dpmn_lds_optin<k_conv_halo_x3<3, 64, 8>>(smem);
  hipLaunchKernelGGL((k_conv_halo_x3<3, 64, 8>), grid, dim3(256), smem, st, a);
  return 0;
}
}  // namespace dpmn_conv

// Instantiates the f32-MFMA (parity mode) variants of the fused contraction: v_mfma_f32_32x32x2_f32.
#include "btx_contract.h"
#include "btx_contract_dma.h"
#include "btx_contract_gemm8.h"
namespace btx {
int launch_contract_f32(int kind, int act_bf16, bool gen, const ContractParams& p, int nwg, hipStream_t st) {
  return launch_contract_impl<0>(kind, act_bf16, gen, p, nwg, st);
}
int launch_contract_var_f32(int var, int act_bf16, bool gen, const ContractParams& p, int nwg, hipStream_t st) {
  return launch_contract_var_impl<0>(var, act_bf16, gen, p, nwg, st);
}
int launch_contract_dma_f32(int kind, const ContractParams& p, int nwg, hipStream_t st) {
  return launch_contract_dma_impl<0>(kind, p, nwg, st);
}
int launch_contract_gemm8_f32(int kind, const ContractParams& p, int nwg, hipStream_t st) {
  return launch_contract_gemm8_impl<0>(kind, p, nwg, st);
}
}  // namespace btx

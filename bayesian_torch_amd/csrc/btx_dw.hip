// btx_dw.hip — the depthwise family (btx_contract_dw.h, BTX-DW v1): its kernels and their launcher.  gfx950 only.
#include "btx_contract_dw.h"

namespace btx {

int launch_contract_dw(int kind, int act_bf16, const ContractParams& p, int nwg, hipStream_t st) {
  return act_bf16 ? launch_contract_dw_impl<__bf16>(kind, p, nwg, st) : launch_contract_dw_impl<float>(kind, p, nwg, st);
}

}  // namespace btx

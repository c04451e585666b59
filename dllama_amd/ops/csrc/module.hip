// dllama_amd — the pybind module: one register_<family>() per source file.

#include "dllama_common.h"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    register_quant_norm(m);
    register_gemv(m);
    register_gemm(m);
    register_attn(m);
    register_moe(m);
    register_sync(m);
    register_sampler(m);
    register_logprob(m);
    register_host(m);
}

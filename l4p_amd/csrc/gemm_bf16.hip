#include "gemm_launch.hpp"
template int launch_gemm_typed<bf16_t>(int mode, const GemmParams& p, hipStream_t stream);
template int launch_gemm_group_typed<bf16_t>(const GemmParams* p, int n, hipStream_t stream);

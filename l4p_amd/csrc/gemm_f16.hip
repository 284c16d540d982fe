// The 16-bit GEMM / conv kernels once more on IEEE half (L4P_F16: the reference's "16-mixed" is fp16 autocast).
#include "gemm_launch.hpp"
template int launch_gemm_typed<f16_t>(int mode, const GemmParams& p, hipStream_t stream);
template int launch_gemm_group_typed<f16_t>(const GemmParams* p, int n, hipStream_t stream);

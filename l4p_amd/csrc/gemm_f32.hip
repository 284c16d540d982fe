#include "gemm_launch.hpp"
template int launch_gemm_typed<float>(int mode, const GemmParams& p, hipStream_t stream);

// explicit instantiation of the MFMA GEMM family for storage dtype bf16_t
#include "gemm_impl.h"
namespace gcv { GCV_INSTANTIATE_GEMM(bf16_t) }

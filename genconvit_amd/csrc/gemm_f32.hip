// explicit instantiation of the MFMA GEMM family for storage dtype float
#include "gemm_impl.h"
namespace gcv { GCV_INSTANTIATE_GEMM(float) }

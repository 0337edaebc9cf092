// explicit instantiation of the MFMA GEMM family for storage dtype half_t
#include "gemm_impl.h"
namespace gcv { GCV_INSTANTIATE_GEMM(half_t) }

GCV_GLDS_STAMP_READER      // (diag/diag.h: nothing unless the build defines GCV_GLDS_STAMPS)

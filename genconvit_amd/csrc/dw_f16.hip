// dw7x7 + LayerNorm: its launcher and band kernels for storage dtype half_t (own TU: built with -fno-slp-vectorize)
#include "dwconv_impl.h"
namespace gcv { GCV_INSTANTIATE_DW(half_t) }

GCV_DW_STAMP_READER      // (diag/diag.h: nothing unless the build defines GCV_DW_STAMPS)

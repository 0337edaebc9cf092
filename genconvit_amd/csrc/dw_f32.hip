// dw7x7 + LayerNorm: its launcher and band kernels for storage dtype float (own TU: built with -fno-slp-vectorize)
#include "dwconv_impl.h"
namespace gcv { GCV_INSTANTIATE_DW(float) }

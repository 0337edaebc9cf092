// dw7x7 + LayerNorm: its launcher and band kernels for storage dtype bf16_t (own TU: built with -fno-slp-vectorize)
#include "dwconv_impl.h"
namespace gcv { GCV_INSTANTIATE_DW(bf16_t) }

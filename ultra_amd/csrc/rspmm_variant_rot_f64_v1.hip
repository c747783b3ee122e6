// Explicit instantiation: RotatE messages, double, the one-element-per-lane fallback (even row lengths that are no multiple
// of 8, unaligned operands): the partner half is loaded.
#include "rspmm_kernels.hpp"
namespace ultra {
ULTRA_DEFINE_ROT_VARIANT(double, 1, 0, false, true)
}  // namespace ultra

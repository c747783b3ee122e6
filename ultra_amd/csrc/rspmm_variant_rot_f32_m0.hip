// Explicit instantiation: RotatE messages, float, operands read through L2 (MODE_GLOBAL), 16-byte lanes: the lane exchange
// (64-element rows) and the loaded partner half (every other row length that is a multiple of 8).
#include "rspmm_kernels.hpp"
namespace ultra {
ULTRA_DEFINE_ROT_VARIANT(float, 4, 0, true, true)
}  // namespace ultra

// Explicit instantiation: RotatE messages, double, operands read through L2 (MODE_GLOBAL), 16-byte lanes: the lane exchange
// (64-element rows) and the loaded partner half (every other row length that is a multiple of 8).
#include "rspmm_kernels.hpp"
namespace ultra {
ULTRA_DEFINE_ROT_VARIANT(double, 4, 0, true, true)
}  // namespace ultra

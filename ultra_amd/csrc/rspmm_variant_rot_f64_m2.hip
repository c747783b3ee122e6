// Explicit instantiation: RotatE messages, double, LDS-staged variant MODE 2 (1: relation slice in LDS, 2: relation + input
// slices in LDS); 64-element rows only, the partner half comes by the lane exchange.
#include "rspmm_kernels.hpp"
namespace ultra {
ULTRA_DEFINE_ROT_VARIANT(double, 4, 2, true, false)
}  // namespace ultra

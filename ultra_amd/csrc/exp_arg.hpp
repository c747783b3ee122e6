// exp(x / T - m) for the self-adversarial weights of the two training losses (loss_kernels.hip, query_train_kernels.hip).
//
// The weight of a negative is softmax(pred / T): exp(x / T - m) / z with m the row's largest x / T.  Formed in plain fp32 the
// argument is rounded twice -- the quotient to 0.5 ulp(|x / T|), the difference to 0.5 ulp(|x / T - m|) -- and either rounding
// is a RELATIVE error of the weight: 2^-18 = 32 ulp of it once the argument passes 64, 256 ulp for a logit of 16 at T = 0.05.
// A negative far below the row's maximum then has a gradient that is wrong in its fifth digit, however exact exp itself is.
//
// Here the argument is carried as an unevaluated sum hi + lo:
//   x / T   is the product with inv_t = fl(1 / T), as the reference's op chain forms it on the GPU (torch divides by a scalar
//           that way); fmaf recovers the product's rounding error exactly:  x inv_t = ph + pl
//   ph - m  = hi + err exactly (Knuth's two-sum)
//   exp(hi + lo) = exp(hi) (1 + lo) to first order, lo = err + pl, |lo| <= ulp(|argument|) < 2^-16 for every argument whose
//           weight is not zero in fp32: the second-order term is below 2^-33.
// m must be the maximum of the same products x * inv_t, so that hi <= 0.
#pragma once
#include <hip/hip_runtime.h>

namespace ultra {

__device__ __forceinline__ float exp_scaled_minus(const float x, const float inv_t, const float m) {
    const float ph = x * inv_t, pl = fmaf(x, inv_t, -ph);
    const float hi = ph - m;
    const float bb = hi - ph;
    const float err = (ph - (hi - bb)) + (-m - bb);
    const float e = expf(hi);
    return fmaf(e, err + pl, e);
}

}  // namespace ultra

// A-direct convolution kernels, stride 2 instances (see conv_ad_kernel.inc; split from conv.hip for build time).
#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "conv_internal.h"

namespace eagle {

#include "conv_ad_kernel.inc"

ConvKernel conv_ad_kernel_s2_bn192(int n_res, bool)      // variant 10: 4 Cout groups x 1 pixel group
{
    static const ConvKernel fn[3] = {conv_f16_ad_kernel<4, 1, 0, true>, conv_f16_ad_kernel<4, 1, 1, true>, conv_f16_ad_kernel<4, 1, 2, true>};
    return fn[res_slot(n_res)];
}

ConvKernel conv_ad_kernel_s2_bn96(int n_res, bool)       // variant 11: 2 Cout groups x 2 pixel groups
{
    static const ConvKernel fn[3] = {conv_f16_ad_kernel<2, 2, 0, true>, conv_f16_ad_kernel<2, 2, 1, true>, conv_f16_ad_kernel<2, 2, 2, true>};
    return fn[res_slot(n_res)];
}

}  // namespace eagle

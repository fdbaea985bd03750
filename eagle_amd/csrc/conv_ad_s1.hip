// A-direct convolution kernels, stride 1 instances (see conv_ad_kernel.inc; split from conv.hip for build time).
#include <algorithm>
#include <cstdlib>

#include "common.h"
#include "conv_internal.h"

namespace eagle {

#include "conv_ad_kernel.inc"

ConvKernel conv_ad_kernel_s1_bn192(int n_res, bool)      // variant 8: 4 Cout groups x 1 pixel group
{
    static const ConvKernel fn[3] = {conv_f16_ad_kernel<4, 1, 0, false>, conv_f16_ad_kernel<4, 1, 1, false>, conv_f16_ad_kernel<4, 1, 2, false>};
    return fn[res_slot(n_res)];
}

ConvKernel conv_ad_kernel_s1_bn96(int n_res, bool)       // variant 9: 2 Cout groups x 2 pixel groups
{
    static const ConvKernel fn[3] = {conv_f16_ad_kernel<2, 2, 0, false>, conv_f16_ad_kernel<2, 2, 1, false>, conv_f16_ad_kernel<2, 2, 2, false>};
    return fn[res_slot(n_res)];
}

}  // namespace eagle

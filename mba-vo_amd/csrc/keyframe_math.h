// keyframe_math.h -- the semi-dense detector's per-pixel device functions, shared by the per-image kernels (keyframe_ops.hip) and
// the batched ones (pairs_prep.hip) so that both compute the same bits from one definition.
#ifndef MBAVO_KEYFRAME_MATH_H
#define MBAVO_KEYFRAME_MATH_H
#include <hip/hip_runtime.h>

namespace mbavo
{
    __device__ __forceinline__ float gradient_magnitude(const unsigned char *__restrict__ src, int H, int W, int x, int y)
    {
        if (x == 0 || y == 0 || x == W - 1 || y == H - 1) return 0.f;
        const size_t i = (size_t)y * W + x;
        const float dx = 0.5f * ((float)src[i + 1] - (float)src[i - 1]);
        const float dy = 0.5f * ((float)src[i + W] - (float)src[i - W]);
        // dx, dy are multiples of 0.5 in [-127.5, 127.5]: the sum of squares is exact in fp32 whatever the
        // contraction; the reference takes the double sqrt of that float and rounds to float, which equals the
        // correctly rounded float sqrt (53 >= 2*24 + 2 bits).  sqrtf is the IEEE one here (hipcc's default
        // -fhip-fp32-correctly-rounded-divide-sqrt); __fsqrt_rn maps to the 1-ulp native instruction.
        return sqrtf(dx * dx + dy * dy);
    }

    // level-0 depth of a level-`lv` pixel (blur_aware_direct_tracker.cpp:398-400): int(x * 2^lv + 0.5)
    __device__ __forceinline__ bool depth_of(const float *__restrict__ depth, int W0, double scale, int x, int y, float &z)
    {
        const int x0 = (int)((float)x * scale + 0.5), y0 = (int)((float)y * scale + 0.5);
        z = depth[(size_t)y0 * W0 + x0];
        return !((double)z < 1e-2);
    }
} // namespace mbavo

#endif

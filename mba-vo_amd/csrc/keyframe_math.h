// keyframe_math.h -- the semi-dense detector's per-pixel device functions, shared by the per-image kernels (keyframe_ops.hip) and
// the batched ones (pairs_prep.hip) so that both compute the same bits from one definition.
#ifndef MBAVO_KEYFRAME_MATH_H
#define MBAVO_KEYFRAME_MATH_H
#include "camera_math.h"
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

    // ---- depth maps as the datasets store them (include/mbavo.h: mbavo_pairs_opts.depth_format, mbavo_depth_to_z)
    //   0  float z
    //   1  float distance along the viewing ray (Utils::load_depthMap + Utils::convert_ray_d_to_z for a pinhole camera without
    //      distortion, utils/InputOutput.cpp:12-37, utils/Geometry.cpp:11-36)
    //   2  uint16, z = value / unit (blur_aware_direct_tracker.cpp:368-386, "eth3d": unit 5000)
    // The conversion is done for the pixel that is looked up, nothing else of the map is read.
    struct DepthConv
    {
        double fx, fy, cx, cy; // level 0
        float unit, max;       // format 2: units per metre; format 1: > 0: a distance above it is no depth
    };
    template <int FORMAT> struct DepthMap { typedef float elem; };
    template <> struct DepthMap<2> { typedef unsigned short elem; };

    // z of the map element v looked up for the level-0 pixel (x0, y0): the formulas of include/mbavo.h, in double, operation by
    // operation.  (x0, y0) is the pixel whose viewing ray format 1 divides by.
    template <int FORMAT>
    __device__ __forceinline__ float depth_z_of(const typename DepthMap<FORMAT>::elem v, int x0, int y0, const DepthConv &c)
    {
        if constexpr (FORMAT == 1)
        {
#pragma clang fp contract(off)
            float d = v;
            if (c.max > 0.f && d > c.max) d = 0.f;
            const double xn = ((double)x0 - c.cx) / c.fx, yn = ((double)y0 - c.cy) / c.fy;
            const double n = sqrt(xn * xn + yn * yn + 1.0); // (IEEE division and square root: correctly rounded, as numpy's)
            return (float)((double)d * (1.0 / n));
        }
        else if constexpr (FORMAT == 2)
        {
#pragma clang fp contract(off)
            return (float)((double)v / (double)c.unit);
        }
        else
            return v;
    }
    // z at the level-0 pixel (x0, y0) of a W0-wide map
    template <int FORMAT>
    __device__ __forceinline__ float depth_z_at(const typename DepthMap<FORMAT>::elem *__restrict__ map, int W0, int x0, int y0, const DepthConv &c)
    {
        return depth_z_of<FORMAT>(map[(size_t)y0 * W0 + x0], x0, y0, c);
    }

    // level-0 depth of a level-`lv` pixel (blur_aware_direct_tracker.cpp:398-400): int(x * 2^lv + 0.5)
    template <int FORMAT>
    __device__ __forceinline__ bool depth_of(const typename DepthMap<FORMAT>::elem *__restrict__ depth, int W0, double scale, int x, int y,
                                             const DepthConv &c, float &z)
    {
        const int x0 = (int)((float)x * scale + 0.5), y0 = (int)((float)y * scale + 0.5);
        z = depth_z_at<FORMAT>(depth, W0, x0, y0, c);
        return !((double)z < 1e-2);
    }
    __device__ __forceinline__ bool depth_of(const float *__restrict__ depth, int W0, double scale, int x, int y, float &z)
    { // a float z map
        return depth_of<0>(depth, W0, scale, x, y, DepthConv{}, z);
    }

    // ---- depth maps in the geometry of a raw, distorted camera (mbavo_pairs_opts.undistort = 2): the level-0 pixel (x0, y0) of
    // the undistorted image is looked up at the raw pixel nearest to its entry of the H0 x W0 undistortion map; an entry that
    // points nowhere or outside the Hs x Ws raw map is no depth.  Format 1 divides by the ray of (x0, y0): the undistorted pixel's
    // ray is the physical ray.  NoRawDepth (an empty kernel argument) keeps the look-up above as it is.
    struct NoRawDepth
    {
    };
    struct RawDepth
    {
        const float *map_xy; // H0 x W0 interleaved [sx, sy]
        int Hs, Ws;
    };
    __device__ __forceinline__ size_t depth_map_elems(const NoRawDepth &, int H0, int W0) { return (size_t)H0 * W0; }
    __device__ __forceinline__ size_t depth_map_elems(const RawDepth &r, int, int) { return (size_t)r.Hs * r.Ws; }
    template <int FORMAT>
    __device__ __forceinline__ bool depth_of(const typename DepthMap<FORMAT>::elem *__restrict__ depth, int W0, double scale, int x, int y,
                                             const DepthConv &c, const NoRawDepth &, float &z)
    {
        return depth_of<FORMAT>(depth, W0, scale, x, y, c, z);
    }
    template <int FORMAT>
    __device__ __forceinline__ bool depth_of(const typename DepthMap<FORMAT>::elem *__restrict__ depth, int W0, double scale, int x, int y,
                                             const DepthConv &c, const RawDepth &r, float &z)
    {
        const int x0 = (int)((float)x * scale + 0.5), y0 = (int)((float)y * scale + 0.5);
        const float2 s = reinterpret_cast<const float2 *>(r.map_xy)[(size_t)y0 * W0 + x0];
        int xr, yr;
        z = 0.f;
        if (!nearest_raw_pixel(s.x, s.y, r.Hs, r.Ws, xr, yr)) return false;
        z = depth_z_of<FORMAT>(depth[(size_t)yr * r.Ws + xr], x0, y0, c);
        return !((double)z < 1e-2);
    }
} // namespace mbavo

#endif

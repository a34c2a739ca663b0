// camera_math.h -- the cameras of the raw images (include/mbavo.h: mbavo_camera_radtan, mbavo_camera_unified): the per-pixel bodies
// of the undistortion map (Undistort::computePixelMappings, core/image_proc/Undistort.cpp:17-52, through CameraPinhole.cpp:24-42,
// 79-95 or CameraUnified.cpp:23-43, and DistortionRadTan.cpp:26-36), of the bilinear remap, of the nearest raw position of a
// depth look-up and of the inverse camera that takes a caller's raw point into the undistorted image (CameraUnified.cpp:68-103,
// DistortionRadTan.cpp:57-80).  Shared by the stand-alone kernels (keyframe_ops.hip: mbavo_undistort_map, _map_unified,
// mbavo_undistort_u8, _u8_batch, mbavo_undistort_points_batch) and the batched ones (pairs_prep.hip) so that both compute the
// same bits from one definition.  The formulas are those of include/mbavo.h, in double, operation by operation.
#ifndef MBAVO_CAMERA_MATH_H
#define MBAVO_CAMERA_MATH_H
#include <hip/hip_runtime.h>

namespace mbavo
{
    // the undistorted pinhole camera the map is made for (`to`) and the raw camera it points into (`from`)
    struct UndistortCams
    {
        double to_fx, to_fy, to_cx, to_cy;
        double fx, fy, cx, cy; // from
        double k1, k2, p1, p2;
    };

    // the same pair of cameras with a unified (omnidirectional) `from` camera: mirror parameter xi, then the distortion of `c`
    struct UndistortCamsUnified
    {
        UndistortCams c;
        double xi;
    };

    // one camera of a set (include/mbavo.h: mbavo_pairs_camera, validated and laid out for the device): the model tag picks the entry
    struct MapCamera
    {
        UndistortCamsUnified u; // model 1: u.c alone
        int model, pad;         // 1: pinhole + radial-tangential  2: unified
    };

    // the point (x, y) of the raw camera's normalised plane through its distortion (DistortionRadTan.cpp:26-36)
    __device__ __forceinline__ void distorted_point(const UndistortCams &m, double x, double y, double &xd, double &yd)
    {
#pragma clang fp contract(off)
        const double mx2 = x * x, my2 = y * y, mxy = x * y, rho2 = mx2 + my2, rad = m.k1 * rho2 + m.k2 * rho2 * rho2;
        xd = x + x * rad + 2.0 * m.p1 * mxy + m.p2 * (rho2 + 2.0 * mx2);
        yd = y + y * rad + 2.0 * m.p2 * mxy + m.p1 * (rho2 + 2.0 * my2);
    }

    // ... and through the intrinsics: the map entry
    __device__ __forceinline__ float2 distorted_pixel(const UndistortCams &m, double x, double y)
    {
#pragma clang fp contract(off)
        double xd, yd;
        distorted_point(m, x, y, xd, yd);
        return make_float2((float)(m.fx * xd + m.cx), (float)(m.fy * yd + m.cy));
    }

    // where output pixel (c, r) of the `to` camera lies in the raw image
    __device__ __forceinline__ float2 undistort_map_entry(const UndistortCams &m, int c, int r)
    {
#pragma clang fp contract(off)
        const double xn = ((double)c - m.to_cx) / m.to_fx, yn = ((double)r - m.to_cy) / m.to_fy; // unproject at z = 1
        const double x = (xn * 1.0) / (1.0 + 1e-8), y = (yn * 1.0) / (1.0 + 1e-8);               // project: CameraPinhole.cpp:30-31
        return distorted_pixel(m, x, y);
    }

    // the same for a unified raw camera (project: CameraUnified.cpp:28-32; z = 1 never takes its failure branch)
    __device__ __forceinline__ float2 undistort_map_entry(const UndistortCamsUnified &u, int c, int r)
    {
#pragma clang fp contract(off)
        const double xn = ((double)c - u.c.to_cx) / u.c.to_fx, yn = ((double)r - u.c.to_cy) / u.c.to_fy; // unproject at z = 1
        const double X = xn * 1.0, Y = yn * 1.0;
        const double d = sqrt(X * X + Y * Y + 1.0); // (correctly rounded)
        const double rz = 1.0 / (1.0 + u.xi * d);
        return distorted_pixel(u.c, X * rz, Y * rz);
    }

    // a map entry that points somewhere: finite and below 2^30 in magnitude, so that floor() of it (and of it + 0.5) fits an int
    __device__ __forceinline__ bool map_entry_usable(double X, double Y)
    { // (a NaN fails both comparisons)
        return fabs(X) < 1073741824.0 && fabs(Y) < 1073741824.0;
    }

    // one output pixel of the remap: bilinear over the four raw pixels around (sx, sy), 0 outside the Hs x Ws raw image
    __device__ __forceinline__ unsigned char remap_u8(const unsigned char *__restrict__ src, int Hs, int Ws, float sx, float sy)
    {
#pragma clang fp contract(off)
        const double X = (double)sx, Y = (double)sy;
        if (!map_entry_usable(X, Y)) return 0;
        const double fx0 = floor(X), fy0 = floor(Y), ax = X - fx0, ay = Y - fy0;
        const int x0 = (int)fx0, y0 = (int)fy0;
        if (x0 < -1 || y0 < -1 || x0 >= Ws || y0 >= Hs) return 0; // all four taps outside: v = 0
        const bool l = x0 >= 0, r = x0 + 1 < Ws, t = y0 >= 0, b = y0 + 1 < Hs;
        const unsigned char *p = src + (long long)y0 * Ws + x0; // (only the taps inside are dereferenced)
        const double p00 = t && l ? (double)p[0] : 0.0, p01 = t && r ? (double)p[1] : 0.0;
        const double p10 = b && l ? (double)p[Ws] : 0.0, p11 = b && r ? (double)p[Ws + 1] : 0.0;
        const double v = (1.0 - ay) * ((1.0 - ax) * p00 + ax * p01) + ay * ((1.0 - ax) * p10 + ax * p11);
        return (unsigned char)(int)(v + 0.5);
    }

    // the raw pixel nearest to a map entry, for a depth look-up; false: no such pixel in the Hs x Ws raw map
    __device__ __forceinline__ bool nearest_raw_pixel(float sx, float sy, int Hs, int Ws, int &xr, int &yr)
    {
#pragma clang fp contract(off)
        const double X = (double)sx, Y = (double)sy;
        if (!map_entry_usable(X, Y)) return false;
        xr = (int)floor(X + 0.5); yr = (int)floor(Y + 0.5);
        return xr >= 0 && xr < Ws && yr >= 0 && yr < Hs;
    }

    // a map entry whose remap reads raw pixels only: no tap of remap_u8 with a non-zero weight lies outside the Hs x Ws raw image
    // (include/mbavo.h: "valid at level 0" of the clearance mask).  NaN and +-inf fail the comparisons, -0.0 passes.
    __device__ __forceinline__ bool map_entry_valid(float sx, float sy, int Hs, int Ws)
    {
        const double X = (double)sx, Y = (double)sy;
        return 0.0 <= X && X <= (double)(Ws - 1) && 0.0 <= Y && Y <= (double)(Hs - 1);
    }

    // ---- the inverse direction (include/mbavo.h: "the inverse camera"): a point (u, v) of the raw image into the undistorted image
    // of the `to` camera.  CameraPinhole::unproject / CameraUnified::unproject (CameraUnified.cpp:68-103) with
    // DistortionRadTan::undistort (DistortionRadTan.cpp:57-80), in double, operation by operation, the unified model's `float`
    // intermediates included.

    // a caller's raw point that has a pixel: map_entry_valid's rule on doubles.  NaN and +-inf fail, -0.0 passes.
    __device__ __forceinline__ bool raw_point_inside(double u, double v, int Hs, int Ws)
    {
        return 0.0 <= u && u <= (double)(Ws - 1) && 0.0 <= v && v <= (double)(Hs - 1);
    }

    // The inverse of the distortion at p = (px, py): at most five Gauss-Newton steps from q = p.  A step evaluates d(q) and its
    // Jacobian J (DistortionRadTan.cpp:42-54, J10 = J01), e = p - d(q), du = (J^T J)^-1 J^T e in closed form, q += du, and stops
    // after the update iff e.e < 1e-15.  The reference returns whatever it has after five steps; here the point is solved iff the
    // stop test fired and q is finite.  With all four coefficients zero d(q) = q: the first step finds e = 0 and stops.
    __device__ __forceinline__ bool undistorted_point(const UndistortCams &m, double px, double py, double &qx, double &qy)
    {
#pragma clang fp contract(off)
        qx = px; qy = py;
        bool stopped = false;
        for (int step = 0; step < 5 && !stopped; ++step)
        {
            double dx, dy;
            distorted_point(m, qx, qy, dx, dy);
            const double mx2 = qx * qx, my2 = qy * qy, mxy = qx * qy, rho2 = mx2 + my2, rad = m.k1 * rho2 + m.k2 * rho2 * rho2;
            const double J00 = 1.0 + rad + 2.0 * m.k1 * mx2 + 4.0 * m.k2 * mx2 * rho2 + 2.0 * m.p1 * qy + 6.0 * m.p2 * qx;
            const double J01 = 2.0 * m.k1 * mxy + 4.0 * m.k2 * rho2 * mxy + 2.0 * m.p1 * qx + 2.0 * m.p2 * qy;
            const double J10 = J01;
            const double J11 = 1.0 + rad + 2.0 * m.k1 * my2 + 4.0 * m.k2 * my2 * rho2 + 2.0 * m.p2 * qx + 6.0 * m.p1 * qy;
            const double ex = px - dx, ey = py - dy;
            const double a = J00 * J00 + J10 * J10, b = J00 * J01 + J10 * J11, c = J01 * J01 + J11 * J11;
            const double g0 = J00 * ex + J10 * ey, g1 = J01 * ex + J11 * ey;
            const double det = a * c - b * b;
            qx += (c * g0 - b * g1) / det;
            qy += (a * g1 - b * g0) / det;
            stopped = ex * ex + ey * ey < 1e-15;
        }
        return stopped && fabs(qx) <= 1.7976931348623157e308 && fabs(qy) <= 1.7976931348623157e308; // (NaN and +-inf fail)
    }

    // The raw point (u, v) of camera `cam` in the undistorted image: (X, Y), or false and X = Y = NaN where there is no solution --
    // the iteration did not stop, the unified model's beta < 0 or lambda - xi < 0, or the result is not finite.  (X, Y) is the
    // inverse of the object's own map as undistort_map_entry builds it (x = xn / (1 + 1e-8)), not a second projection: the position
    // whose map entry is the raw point.
    __device__ __forceinline__ bool undistorted_position(const MapCamera &cam, double u, double v, double &X, double &Y)
    {
#pragma clang fp contract(off)
        const UndistortCams &m = cam.u.c;
        const double nan = __builtin_nan("");
        double qx, qy;
        bool ok = undistorted_point(m, (u - m.cx) / m.fx, (v - m.cy) / m.fy, qx, qy);
        double x = qx, y = qy;
        if (cam.model == 2)
        { // CameraUnified.cpp:81-99
            const double xi = cam.u.xi;
            const float rho2 = (float)(qx * qx + qy * qy);
            const float beta = (float)(1.0 + (1.0 - xi * xi) * (double)rho2);
            const float lambda = (float)((xi + (double)sqrtf(beta)) / (1.0 + (double)rho2)); // (sqrtf: correctly rounded)
            const double pz = (double)lambda - xi;
            if (beta < 0.f || pz < 0.0) ok = false;
            x = ((double)lambda * qx) / pz;
            y = ((double)lambda * qy) / pz;
        }
        X = m.to_fx * (x * (1.0 + 1e-8)) + m.to_cx;
        Y = m.to_fy * (y * (1.0 + 1e-8)) + m.to_cy;
        ok = ok && fabs(X) <= 1.7976931348623157e308 && fabs(Y) <= 1.7976931348623157e308;
        if (!ok) X = Y = nan;
        return ok;
    }

    // one output byte of the warp of a raw-geometry MASK (include/mbavo.h: "warp of a raw-geometry mask"; a byte != 0 is usable):
    // 1 iff the entry is valid and the raw mask is non-zero at every tap of remap_u8 that carries weight -- (x0, y0) always, its
    // right neighbour iff ax > 0, the one below iff ay > 0, the diagonal one iff both.  A tap of weight 0 is never read.  For a
    // valid entry every tap read lies inside the raw image: X <= Ws - 1 and ax > 0 give x0 + 1 <= Ws - 1, the same for Y; -0.0
    // floors to -0.0 = pixel 0 with ax = 0.
    __device__ __forceinline__ unsigned char warp_mask_u8(const unsigned char *__restrict__ src, int Hs, int Ws, float sx, float sy)
    {
#pragma clang fp contract(off)
        if (!map_entry_valid(sx, sy, Hs, Ws)) return 0;
        const double X = (double)sx, Y = (double)sy;
        const double fx0 = floor(X), fy0 = floor(Y); // (as remap_u8 splits the entry)
        const bool right = X - fx0 > 0.0, below = Y - fy0 > 0.0;
        const unsigned char *p = src + (long long)(int)fy0 * Ws + (int)fx0;
        bool ok = p[0] != 0;
        if (right) ok = ok && p[1] != 0;
        if (below) ok = ok && p[Ws] != 0;
        if (right && below) ok = ok && p[Ws + 1] != 0;
        return ok ? 1 : 0;
    }

    // four adjacent output bytes i0 .. i0 + 3 of a flat H*W mask, as remap_four makes four pixels: two 16-byte map loads and one
    // word stored where the map and the destination allow it, byte by byte otherwise.  The same bytes either way.
    __device__ __forceinline__ void warp_mask_four(const unsigned char *__restrict__ src, int Hs, int Ws, const float *__restrict__ map,
                                                   unsigned char *__restrict__ dst, int npx, int i0)
    {
        const float *m = map + 2 * (size_t)i0;
        if (i0 + 4 <= npx && (((size_t)m & 15) | ((size_t)(dst + i0) & 3)) == 0)
        {
            const float4 a = reinterpret_cast<const float4 *>(m)[0], b = reinterpret_cast<const float4 *>(m)[1];
            const unsigned v0 = warp_mask_u8(src, Hs, Ws, a.x, a.y), v1 = warp_mask_u8(src, Hs, Ws, a.z, a.w);
            const unsigned v2 = warp_mask_u8(src, Hs, Ws, b.x, b.y), v3 = warp_mask_u8(src, Hs, Ws, b.z, b.w);
            *reinterpret_cast<unsigned *>(dst + i0) = v0 | (v1 << 8) | (v2 << 16) | (v3 << 24);
        }
        else
            for (int j = 0; j < 4 && i0 + j < npx; ++j) dst[i0 + j] = warp_mask_u8(src, Hs, Ws, m[2 * j], m[2 * j + 1]);
    }

    // four adjacent output pixels i0 .. i0 + 3 of N flat H*W images that go through the SAME map entries (N = 1: an image; N = 2:
    // both images of a pair), the entries loaded once.  Stored as one word per image where the destinations and the map allow it
    // (every dst 4-byte, map 16-byte aligned at i0, four pixels left), byte by byte otherwise (the ragged end, a caller's unaligned
    // buffer).  The branch is uniform but for the last lane of the image.  The same bytes for an image whatever N is.
    template <int N>
    __device__ __forceinline__ void remap_four(const unsigned char *const (&src)[N], int Hs, int Ws, const float *__restrict__ map,
                                               unsigned char *const (&dst)[N], int npx, int i0)
    {
        const float *m = map + 2 * (size_t)i0;
        size_t off = (size_t)m & 15;
#pragma unroll
        for (int n = 0; n < N; ++n) off |= (size_t)(dst[n] + i0) & 3;
        if (i0 + 4 <= npx && off == 0)
        {
            const float4 a = reinterpret_cast<const float4 *>(m)[0], b = reinterpret_cast<const float4 *>(m)[1];
            unsigned word[N];
#pragma unroll
            for (int n = 0; n < N; ++n)
            {
                const unsigned v0 = remap_u8(src[n], Hs, Ws, a.x, a.y), v1 = remap_u8(src[n], Hs, Ws, a.z, a.w);
                const unsigned v2 = remap_u8(src[n], Hs, Ws, b.x, b.y), v3 = remap_u8(src[n], Hs, Ws, b.z, b.w);
                word[n] = v0 | (v1 << 8) | (v2 << 16) | (v3 << 24);
            }
#pragma unroll
            for (int n = 0; n < N; ++n) *reinterpret_cast<unsigned *>(dst[n] + i0) = word[n];
        }
        else
            for (int j = 0; j < 4 && i0 + j < npx; ++j)
            {
                const float sx = m[2 * j], sy = m[2 * j + 1];
#pragma unroll
                for (int n = 0; n < N; ++n) dst[n][i0 + j] = remap_u8(src[n], Hs, Ws, sx, sy);
            }
    }
} // namespace mbavo

#endif

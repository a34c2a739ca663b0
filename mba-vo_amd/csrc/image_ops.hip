// image_ops.hip -- keyframe input producers on device: 2x2 box pyramid level and
// central-difference gradient image (core/measurements/ImagePyramid.h:59-99,
// core/image_proc/Gradient.h:16-75).  Pure streaming kernels (HBM-bound).  The gradient image's three formats are one
// kernel over the pixel's differences and encoders of keyframe_math.h, which the batched gradients (pairs_prep.hip) call too.
#include "../../include/mbavo.h"
#include "host_math.h"
#include "keyframe_math.h"
#include <hip/hip_runtime.h>
#include <vector>

namespace mbavo
{
    // dst(h,w) = uchar(0.25f * (a + b + c + d)), truncation toward zero (ImagePyramid.h:86-91);
    // the four uint8 sum exactly in float and 0.25 scaling is exact, so this is (a+b+c+d) >> 2.
    __global__ void k_pyr_down(const unsigned char *__restrict__ src, int W, int Hl, int Wl,
                               unsigned char *__restrict__ dst)
    {
        const int w = blockIdx.x * blockDim.x + threadIdx.x, h = blockIdx.y;
        if (w >= Wl || h >= Hl) return;
        const unsigned char *r0 = src + (size_t)(2 * h) * W + 2 * w;
        const unsigned char *r1 = r0 + W;
        const int s = (int)r0[0] + (int)r0[1] + (int)r1[0] + (int)r1[1];
        dst[(size_t)h * Wl + w] = (unsigned char)(s >> 2);
    }

    // central-difference gradient image of one level, one pixel per lane in the keyframe format FORMAT (keyframe_math.h:
    // central_diff, GradPixel); a store of the pixel's own size: a caller's buffer need not be 16-byte aligned
    template <int FORMAT>
    __global__ void k_gradients(const unsigned char *__restrict__ src, int H, int W, typename GradPixel<FORMAT>::type *__restrict__ g)
    {
        const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
        if (x >= W || y >= H) return;
        const size_t i = (size_t)y * W + x;
        int kx, ky;
        central_diff(src, H, W, x, y, i, kx, ky);
        g[i] = GradPixel<FORMAT>::of((int)src[i], kx, ky);
    }
    template <int FORMAT> static int gradients_u8(const unsigned char *d_src, int H, int W, void *d_out, void *stream)
    {
        if (!d_src || !d_out || H < 1 || W < 1) return MBAVO_E_ARG;
        hipLaunchKernelGGL(k_gradients<FORMAT>, dim3((W + 255) / 256, H), dim3(256), 0, (hipStream_t)stream, d_src, H, W,
                           (typename GradPixel<FORMAT>::type *)d_out);
        return (int)hipGetLastError();
    }
    // Synthetic motion blur (generate_synthetic_data.cpp:127-214): every output pixel is warped into the sharp
    // image through each of the n sampled poses, every warp is truncated to 8 bits as warp_image() stores it, the n
    // images are averaged in float and rounded to nearest even like cv::Mat::convertTo(CV_8U).
    // The warp follows compute_pixel_intensity.h:113-144 operation by operation, without FMA contraction, so the
    // generator is bit-identical to the CPU one (a 1e-13 difference in the tap coordinate can flip an 8-bit
    // truncation); this is input synthesis, not the hot path, so the extra flops do not matter.
    __global__ void k_synth_blur(const unsigned char *__restrict__ ref, int H, int W, double D, double fx, double fy,
                                 double cx, double cy, const double *__restrict__ poses /*n x 7*/, int n,
                                 unsigned char *__restrict__ out)
    {
#pragma clang fp contract(off)
        const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
        if (c >= W || r >= H) return;
        double xh = ((double)c - cx) / fx;
        double yh = ((double)r - cy) / fy;
        const double zh = 1. / (double)sqrtf((float)(1. + xh * xh + yh * yh));
        xh *= zh;
        yh *= zh;
        float acc = 0.f;
        for (int i = 0; i < n; ++i)
        {
            const double *p = poses + 7 * i;
            const double x = p[0], y = p[1], z = p[2], qx = p[3], qy = p[4], qz = p[5], qw = p[6];
            const double lambda = 2. * xh * (qx * qz - qw * qy) + 2. * yh * (qx * qw + qy * qz) +
                                  zh * (qw * qw - qx * qx - qy * qy + qz * qz);
            const double s = (D - z) / lambda;
            const double pc[3] = {s * xh, s * yh, s * zh};
            double pr[3];
            qrotate(Quat{qx, qy, qz, qw}, pc, pr);
            const double Px = pr[0] + x, Py = pr[1] + y, Pz = pr[2] + z;
            const double iz = 1. / (Pz + 1e-8);
            const double u = fx * (Px * iz) + cx, v = fy * (Py * iz) + cy;
            double val = 0.0, gx, gy;
            if (!bilinear_tap<false>(ref, nullptr, H, W, u, v, val, gx, gy)) val = 0.0;
            acc = acc + (float)(unsigned char)val;
        }
        const float m = acc / (float)n;
        int q = (int)rintf(m);
        q = q < 0 ? 0 : (q > 255 ? 255 : q);
        out[(size_t)r * W + c] = (unsigned char)q;
    }
} // namespace mbavo

extern "C" int mbavo_synthesize_blur(const unsigned char *d_ref, int H, int W, double plane_depth, const double intr[4],
                                     int k, double t0, double dt, const double *h_knots_t, const double *h_knots_R, int N,
                                     double cap, double exp_t, int num_samples, unsigned char *d_out, void *stream)
{
    if (!d_ref || !d_out || !intr || !h_knots_t || !h_knots_R || (k != 2 && k != 4) || num_samples < 2 || H < 2 || W < 2)
        return MBAVO_E_ARG;
    SLAM::Core::SplineSE3 spline(t0, dt);
    spline.setSplineDegK(k);
    for (int i = 0; i < N; ++i) spline.InsertControlKnot(h_knots_R + 4 * i, h_knots_t + 3 * i);
    std::vector<double> poses((size_t)num_samples * 7);
    for (int i = 0; i < num_samples; ++i)
    { // sample times of synthesize_motion_blurred_img (:201): cap - exp/2 + i*exp/(n-1)
        const double t = cap - exp_t * 0.5 + i * exp_t / (num_samples - 1);
        if (!spline.GetPose(t, &poses[7 * i + 3], &poses[7 * i])) return MBAVO_E_RANGE;
    }
    double *d_poses = nullptr;
    hipError_t e = hipMalloc((void **)&d_poses, poses.size() * sizeof(double));
    if (e != hipSuccess) return (int)e;
    e = hipMemcpyAsync(d_poses, poses.data(), poses.size() * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess)
    {
        hipLaunchKernelGGL(mbavo::k_synth_blur, dim3((W + 127) / 128, H), dim3(128), 0, (hipStream_t)stream, d_ref, H, W,
                           plane_depth, intr[0], intr[1], intr[2], intr[3], d_poses, num_samples, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    (void)hipFree(d_poses);
    return (int)e;
}

extern "C" int mbavo_image_gradients_u8_half(const unsigned char *d_src, int H, int W, void *d_dIxy_half, void *stream)
{
    return mbavo::gradients_u8<1>(d_src, H, W, d_dIxy_half, stream);
}

extern "C" int mbavo_pack_keyframe_u8(const unsigned char *d_src, int H, int W, void *d_packed, void *stream)
{
    return mbavo::gradients_u8<2>(d_src, H, W, d_packed, stream);
}

extern "C" int mbavo_pyramid_down_u8(const unsigned char *d_src, int H, int W, unsigned char *d_dst, void *stream)
{
    if (!d_src || !d_dst || H < 2 || W < 2) return MBAVO_E_ARG;
    const int Hl = H / 2, Wl = W / 2;
    hipLaunchKernelGGL(mbavo::k_pyr_down, dim3((Wl + 255) / 256, Hl), dim3(256), 0, (hipStream_t)stream, d_src, W, Hl, Wl, d_dst);
    return (int)hipGetLastError();
}

extern "C" int mbavo_image_gradients_u8(const unsigned char *d_src, int H, int W, float *d_dIxy, void *stream)
{
    return mbavo::gradients_u8<0>(d_src, H, W, d_dIxy, stream);
}

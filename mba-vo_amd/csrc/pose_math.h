// pose_math.h -- 7-double poses [t | q xyzw] (Core::Transformation) and the SE(3) exponential / logarithm for the kernels that
// carry tracker state from frame to frame (pairs_track.hip: k_pairs_predict, k_pairs_commit).  Host + device, header only; beside
// so3_exp / qlog of se3_math.h, whose sine / cosine / arctangent forms they use on the device.
#ifndef MBAVO_POSE_MATH_H
#define MBAVO_POSE_MATH_H

#include "se3_math.h"

namespace mbavo
{
    // They restate vo_frontend.cpp's Transformation operation for operation, without contraction (the host build has no FMA).  On
    // the device the sine / cosine and the arctangent are se3_math.h's fastm forms (sine and cosine within 1.93, the arctangent within 2.8 units in the last place of the
    // correctly rounded value -- measured 1.30 / 1.42 and 2.32, so NOT the "one or two" of se3_math.h's comment for the arctangent --
    // and next to a multiple of pi/2 |k| * 3.52e-27 absolute more, which is any number of units of the small one of sine and cosine:
    // derived and held in tests/harness/fastm_check.hip, figures in profiles/r41_fastm.txt);
    // square roots and divisions are the correctly rounded ones on both sides: one lane walks this once per frame, and every
    // quotient that keeps the host's bits is a result that needs no tolerance.
    MBAVO_HD void pose_make(const Quat &q, const double t[3], double T[7])
    { // Core::Transformation(q, t): Eigen normalized()
#pragma clang fp contract(off)
        const double z = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
        double n = 1.0;
        if (z > 0) n = sqrt(z);
        T[0] = t[0]; T[1] = t[1]; T[2] = t[2];
        T[3] = z > 0 ? q.x / n : q.x; T[4] = z > 0 ? q.y / n : q.y; T[5] = z > 0 ? q.z / n : q.z; T[6] = z > 0 ? q.w / n : q.w;
    }
    MBAVO_HD void pose_inverse(const double T[7], double Ti[7])
    { // Transformation.cpp:83-90
        const Quat qc{-T[3], -T[4], -T[5], T[6]};
        const double nt[3] = {-T[0], -T[1], -T[2]};
        double ti[3];
        qrotate(qc, nt, ti);
        pose_make(qc, ti, Ti);
    }
    MBAVO_HD void pose_mul(const double A[7], const double B[7], double out[7])
    { // operator* (Transformation.cpp:109-119)
        const Quat a = load_quat(A + 3);
        const Quat q = qmul(a, load_quat(B + 3));
        double t[3];
        qrotate(a, B, t);
        t[0] += A[0]; t[1] += A[1]; t[2] += A[2];
        pose_make(q, t, out);
    }
    MBAVO_HD void hat_and_square(const double w[3], double O[9], double O2[9])
    {
#pragma clang fp contract(off)
        const double h[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
#pragma unroll
        for (int i = 0; i < 9; ++i) O[i] = h[i];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
            {
                double a = 0;
#pragma unroll
                for (int j = 0; j < 3; ++j) a += h[r * 3 + j] * h[j * 3 + c];
                O2[r * 3 + c] = a;
            }
    }
    MBAVO_HD void se3_exp(const double a[6], double T[7])
    { // Transformation::exp (Transformation.cpp:171-177 -> Sophus::SE3d::exp): t = V(omega) * upsilon
#pragma clang fp contract(off)
        const double *om = a + 3;
        const Quat q = so3_exp(om);
        const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
        double O[9], O2[9], V[9];
        hat_and_square(om, O, O2);
        if (theta < 1e-10)
        {
            const double x = q.x, y = q.y, z = q.z, w = q.w; // V = so3.matrix()
            const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                                 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                                 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
#pragma unroll
            for (int i = 0; i < 9; ++i) V[i] = R[i];
        }
        else
        {
            const double th2 = theta * theta;
#if defined(MBAVO_POSE_FASTMATH)
            double sn, cs;
            fastm::sincos(theta, sn, cs);
#else
            const double sn = sin(theta), cs = cos(theta);
#endif
            const double c1 = (1 - cs) / th2, c2 = (theta - sn) / (th2 * theta);
#pragma unroll
            for (int i = 0; i < 9; ++i) V[i] = ((i % 4 == 0) ? 1.0 : 0.0) + c1 * O[i] + c2 * O2[i];
        }
        double t[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) t[r] = V[r * 3] * a[0] + V[r * 3 + 1] * a[1] + V[r * 3 + 2] * a[2];
        pose_make(q, t, T);
    }
    MBAVO_HD void se3_log(const double T[7], double out[6])
    { // Transformation::log (Transformation.cpp:164-169 -> Sophus::SE3d::log)
#pragma clang fp contract(off)
        const double *q = T + 3, *t = T;
        const double sn = q[0] * q[0] + q[1] * q[1] + q[2] * q[2], w = q[3], n = sqrt(sn);
        double two_atan;
        if (sn < 1e-10 * 1e-10)
            two_atan = 2.0 / w - 2.0 * sn / (w * (w * w));
        else if (fabs(w) < 1e-10)
            two_atan = (w > 0 ? 3.14159265358979323846 : -3.14159265358979323846) / n;
        else
#if defined(MBAVO_POSE_FASTMATH)
            two_atan = 2.0 * fastm::atan_ratio(n, w) / n;
#else
            two_atan = 2.0 * atan(n / w) / n;
#endif
        const double theta = two_atan * n;
        const double om[3] = {two_atan * q[0], two_atan * q[1], two_atan * q[2]};
        double O[9], O2[9];
        hat_and_square(om, O, O2);
        double c2;
        if (fabs(theta) < 1e-10)
            c2 = 1.0 / 12.0;
        else
        {
            const double h = 0.5 * theta;
#if defined(MBAVO_POSE_FASTMATH)
            double sh, ch;
            fastm::sincos(h, sh, ch);
#else
            const double sh = sin(h), ch = cos(h);
#endif
            c2 = (1 - theta * ch / (2 * sh)) / (theta * theta);
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
        {
            double acc = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc += (((r == c) ? 1.0 : 0.0) - 0.5 * O[r * 3 + c] + c2 * O2[r * 3 + c]) * t[c];
            out[r] = acc;
        }
        out[3] = om[0]; out[4] = om[1]; out[5] = om[2];
    }
} // namespace mbavo

#endif

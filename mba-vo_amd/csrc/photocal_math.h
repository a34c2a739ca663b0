// photocal_math.h -- the photometric calibration of a raw image (include/mbavo.h: mbavo_pairs_set_photometric,
// mbavo_photometric_u8_batch): the per-pixel bodies of the inverse vignette, of the calibrated tap, of the calibrated pinhole intake
// and of the calibrated remap.  Shared by the batched kernels of the pairs object and the stand-alone call (pairs_photocal.hip) so
// that both compute the same bits from one definition.  The formulas are those of include/mbavo.h: a tap is the product of two
// floats formed in double (exact), the blend is camera_math.h's remap_u8 with every dereferenced tap replaced by it.
#ifndef MBAVO_PHOTOCAL_MATH_H
#define MBAVO_PHOTOCAL_MATH_H
#include "camera_math.h"

namespace mbavo
{
    // one entry of the inverse vignette: 1 / V in float where the vignette says something, 0 (black) elsewhere.  The quotient is
    // formed in double and rounded once more: 53 >= 2 * 24 + 2 bits, so the result is the correctly rounded float quotient whatever
    // the build's float division is.  NaN and +-inf fail the first comparison.
    __device__ __forceinline__ float inverse_vignette(float V, float v_min)
    {
        return (fabsf(V) <= 3.4028234663852886e38f && V >= v_min) ? (float)(1.0 / (double)V) : 0.0f;
    }

    // VIG, the inverse vignette a tap is scaled with: NoVignette (V == NULL: 1.0f everywhere, no map read, no code) or Vignette,
    // the float map of the image's calibration in the geometry the image arrives in
    struct NoVignette
    {
        __device__ __forceinline__ double at(long long) const { return 1.0; }
        __device__ __forceinline__ size_t misaligned(int) const { return 0; }
    };
    struct Vignette
    {
        const float *inv;
        __device__ __forceinline__ double at(long long i) const { return (double)inv[i]; }
        __device__ __forceinline__ size_t misaligned(int i0) const { return (size_t)(inv + i0) & 15; }
    };

    // t = (double)lut[raw] * (double)inv: grey level `raw` of pixel i of the arriving image as scaled irradiance
    template <class VIG>
    __device__ __forceinline__ double photocal_tap(const float *lut, const VIG &vig, unsigned raw, long long i)
    {
        return (double)lut[raw] * vig.at(i);
    }

    // the byte the object stores for a value v >= 0 (a NaN, which 0 * inf gives under a v_min below 1 / FLT_MAX, saturates)
    __device__ __forceinline__ unsigned char photocal_u8(double v) { return (unsigned char)(int)(fmin(v, 255.0) + 0.5); }

    // ---- pinhole intake: sixteen adjacent pixels i0 .. i0 + 15 of a flat image of npx pixels.  One 16-byte store (four word loads
    // of the source, four 16-byte loads of the vignette) where the pointers allow it -- the source on a word, destination and
    // vignette on 16 bytes at i0, sixteen pixels left --, byte by byte otherwise (the ragged end, a caller's unaligned buffer, the
    // vignette of a later calibration where npx is no multiple of 4).  Every source byte is read before the store: dst == src is
    // allowed.  The same bytes either way.
    template <class VIG>
    __device__ __forceinline__ void photocal_sixteen(const unsigned char *src, const float *lut, const VIG &vig, unsigned char *dst, int npx, int i0)
    {
        const size_t off = ((size_t)(src + i0) & 3) | ((size_t)(dst + i0) & 15) | vig.misaligned(i0);
        if (i0 + 16 <= npx && off == 0)
        {
            const unsigned *s4 = reinterpret_cast<const unsigned *>(src + i0);
            const unsigned in[4] = {s4[0], s4[1], s4[2], s4[3]};
            unsigned out[4];
#pragma unroll
            for (int w = 0; w < 4; ++w)
            {
                unsigned word = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    word |= (unsigned)photocal_u8(photocal_tap(lut, vig, (in[w] >> (8 * j)) & 255u, i0 + 4 * w + j)) << (8 * j);
                out[w] = word;
            }
            *reinterpret_cast<uint4 *>(dst + i0) = make_uint4(out[0], out[1], out[2], out[3]);
        }
        else
            for (int j = 0; j < 16 && i0 + j < npx; ++j) dst[i0 + j] = photocal_u8(photocal_tap(lut, vig, src[i0 + j], i0 + j));
    }

    // ---- raw intake: remap_u8 with every dereferenced tap p_ij replaced by the calibrated tap at that raw pixel; the usability and
    // outside rules stay, the blend's order stays
    template <class VIG>
    __device__ __forceinline__ unsigned char remap_u8_cal(const unsigned char *__restrict__ src, int Hs, int Ws, float sx, float sy,
                                                          const float *lut, const VIG &vig)
    {
#pragma clang fp contract(off)
        const double X = (double)sx, Y = (double)sy;
        if (!map_entry_usable(X, Y)) return 0;
        const double fx0 = floor(X), fy0 = floor(Y), ax = X - fx0, ay = Y - fy0;
        const int x0 = (int)fx0, y0 = (int)fy0;
        if (x0 < -1 || y0 < -1 || x0 >= Ws || y0 >= Hs) return 0; // all four taps outside: v = 0
        const bool l = x0 >= 0, r = x0 + 1 < Ws, t = y0 >= 0, b = y0 + 1 < Hs;
        const long long o = (long long)y0 * Ws + x0; // (only the taps inside are dereferenced, in the image and in the vignette)
        const double p00 = t && l ? photocal_tap(lut, vig, src[o], o) : 0.0, p01 = t && r ? photocal_tap(lut, vig, src[o + 1], o + 1) : 0.0;
        const double p10 = b && l ? photocal_tap(lut, vig, src[o + Ws], o + Ws) : 0.0;
        const double p11 = b && r ? photocal_tap(lut, vig, src[o + Ws + 1], o + Ws + 1) : 0.0;
        const double v = (1.0 - ay) * ((1.0 - ax) * p00 + ax * p01) + ay * ((1.0 - ax) * p10 + ax * p11);
        return photocal_u8(v);
    }

    // remap_four of camera_math.h under the tap policy above: four adjacent output pixels of N images that go through the SAME map
    // entries and the SAME calibration (N = 2: both images of a pair), one word per image where destinations and map allow it
    template <int N, class VIG>
    __device__ __forceinline__ void remap_four_cal(const unsigned char *const (&src)[N], int Hs, int Ws, const float *__restrict__ map,
                                                   const float *lut, const VIG &vig, unsigned char *const (&dst)[N], int npx, int i0)
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
                const unsigned v0 = remap_u8_cal(src[n], Hs, Ws, a.x, a.y, lut, vig), v1 = remap_u8_cal(src[n], Hs, Ws, a.z, a.w, lut, vig);
                const unsigned v2 = remap_u8_cal(src[n], Hs, Ws, b.x, b.y, lut, vig), v3 = remap_u8_cal(src[n], Hs, Ws, b.z, b.w, lut, vig);
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
                for (int n = 0; n < N; ++n) dst[n][i0 + j] = remap_u8_cal(src[n], Hs, Ws, sx, sy, lut, vig);
            }
    }
} // namespace mbavo

#endif

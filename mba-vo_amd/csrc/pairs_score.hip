// pairs_score.hip -- keypoints by corner strength (include/mbavo.h: mbavo_corner_score_u8, mbavo_pairs_set_detector,
// mbavo_pairs_detector_stats).  The response is the minimum eigenvalue of the windowed structure tensor, the score of the
// reference's ENUM_SPARSE_SHI_TOMASI detector (FeatureDetectorSparse.cpp, cv::goodFeaturesToTrack on the CPU), used under the
// project's own selection: the grid cells or every candidate of pairs_prep.hip, which read it through a response policy.
//
// The score (the definition; keyframe_math.h: corner_score_of_sums, corner_score_tile compute it).  For a level image I of H x W
// bytes, a pixel (x, y) and a radius r in {1, 2, 3}:
//   kx, ky   are central_diff of keyframe_math.h: right - left and bottom - top as integers, zero on the 1-pixel border
//   a = sum kx^2, b = sum kx ky, c = sum ky^2, summed over the (2r+1) x (2r+1) window centred on the pixel
//            - window positions outside the image contribute 0
//            - n = (2r+1)^2 always; there is no renormalisation at the border
//            - all three sums are exact in int (|a|, |b|, |c| <= 49 * 255^2)
//   in double, with contraction off:
//            tr = (double)(a + c)
//            s  = sqrt((double)(a-c) * (double)(a-c) + 4.0 * (double)b * (double)b); the argument is an exact integer below 2^53
//            d  = tr - s, and d = 0 where d < 0
//            score = (float)sqrt(d / (8.0 * n))
// This is the RMS gradient along the weakest direction of the window, in grey levels per pixel.  It is the unit of
// gradient_magnitude, so a threshold means the same kind of thing in both modes.  Every operation is exact or one correctly
// rounded IEEE operation; numpy gives the same bits (tests/pairs_score_ref.py), so every test is an equality.
//   A constant image scores 0 everywhere.  An image with ky = 0 everywhere, such as a vertical step edge, scores exactly 0
//   everywhere, because s = a exactly.  An image with kx = ky everywhere scores exactly 0, because s = 2a exactly.
// A pixel is a candidate iff score > threshold, strictly; grid selection keeps the first pixel in row-major order with the
// strictly largest score in its cell.
//
// ONE launch scores every level of every keyframe that changed, indexed the way k_pairs_gradients is: the levels' tiles side by
// side in blockIdx.x (a PairsGrid whose blk0 counts tiles), the pair's row in blockIdx.y, pair_of_row for updates.  A workgroup of
// 256 takes one 16 x 32 tile of a level through LDS (corner_score_tile) and writes one float per pixel into the (pair, level)'s
// score slice.  The radius is a template parameter: the window loops unroll, the LDS arrays are sized for it.
#include "pairs_prep.h"
#include "keyframe_math.h"
#include "pairs_desc.h"
#include <climits>
#include <cmath>
#include <cstring>
#include <hip/hip_runtime.h>

namespace mbavo
{
    namespace pairs
    {
        template <int R>
        __global__ __launch_bounds__(256) void k_corner_score(const unsigned char *__restrict__ src, int H, int W, float *__restrict__ score)
        {
            const int tiles_w = (W + kScoreTileW - 1) / kScoreTileW, ty = (int)blockIdx.x / tiles_w, tx = (int)blockIdx.x - ty * tiles_w;
            corner_score_tile<R>(src, H, W, tx * kScoreTileW, ty * kScoreTileH, score);
        }

        template <int R>
        __global__ __launch_bounds__(256) void k_pairs_score(const PairLevelDesc *__restrict__ desc, const PairsGrid g,
                                                             const int *__restrict__ key_pairs, const ScoreSlices slices)
        {
            const int pair = pair_of_row(key_pairs, (int)blockIdx.y);
            int l = 0;
            while (l + 1 < g.L && (int)blockIdx.x >= g.blk0[l + 1]) ++l;
            const PairLevelDesc &d = desc[(size_t)pair * g.L + l];
            const int t = (int)blockIdx.x - g.blk0[l], tiles_w = (d.W + kScoreTileW - 1) / kScoreTileW, ty = t / tiles_w, tx = t - ty * tiles_w;
            corner_score_tile<R>(d.ref, d.H, d.W, tx * kScoreTileW, ty * kScoreTileH, slices.of(d));
        }

        static long long score_tiles(int H, int W)
        {
            return (long long)((H + kScoreTileH - 1) / kScoreTileH) * (long long)((W + kScoreTileW - 1) / kScoreTileW);
        }
    } // namespace pairs

    using namespace pairs;

    // Pure host: nothing is allocated before the options have passed, and an object that never asks holds nothing.
    int PairBatch::set_detector(const mbavo_pairs_detector_opts *o)
    {
        if (!arena_) return MBAVO_E_ARG;
        const mbavo_pairs_detector_opts none{};
        if (!o) o = &none;
        for (int r : o->reserved)
            if (r != 0) return MBAVO_E_ARG;
        if (o->score != 0 && o->score != 1) return MBAVO_E_ARG;
        if (o->score == 0)
        { // (the slices stay: a later score = 1 finds them)
            detector_.score = 0; detector_.radius = 0; detector_.threshold = 0.f;
            return 0;
        }
        if (o->radius < 1 || o->radius > 3 || !std::isfinite(o->score_threshold) || o->score_threshold < 0.f) return MBAVO_E_ARG;
        if (!detector_.slices)
        { // 4 bytes per gradient pixel of every pair: grad_stride is a multiple of 256 bytes, grad_bytes 4 or 8
            hipError_t e = hipSetDevice(eng_.device());
            if (e != hipSuccess) return (int)e;
            const long long bytes = (long long)plan_.B * (plan_.grad_stride / plan_.grad_bytes) * (long long)sizeof(float);
            if ((e = detector_.slices.alloc((size_t)bytes)) != hipSuccess) return (int)e;
            detector_.bytes = bytes;
        }
        detector_.score = 1; detector_.radius = o->radius; detector_.threshold = o->score_threshold;
        return 0;
    }

    ScoreSlices PairBatch::score_slices() const { return ScoreSlices{detector_.slices.p, lay_.grad(arena_), plan_.grad_bytes == 8 ? 3 : 2}; }

    void PairBatch::score_levels(int n_key, const int *d_keys, CallStats &s)
    {
        const PairsPlan &p = plan_;
        PairsGrid g;
        memset(&g, 0, sizeof(g));
        g.L = p.L; g.B = p.B;
        for (int l = 0; l < p.L; ++l) g.blk0[l + 1] = g.blk0[l] + (int)score_tiles(p.H[l], p.W[l]); // (at most 2^22 pixels a level)
        const dim3 grid(g.blk0[p.L], n_key);
        const PairLevelDesc *desc = lay_.desc(arena_);
        const ScoreSlices sl = score_slices();
        hipStream_t st = eng_.stream();
        if (detector_.radius == 1) hipLaunchKernelGGL(k_pairs_score<1>, grid, dim3(256), 0, st, desc, g, d_keys, sl);
        else if (detector_.radius == 2) hipLaunchKernelGGL(k_pairs_score<2>, grid, dim3(256), 0, st, desc, g, d_keys, sl);
        else hipLaunchKernelGGL(k_pairs_score<3>, grid, dim3(256), 0, st, desc, g, d_keys, sl);
        ++s.launches;
    }
} // namespace mbavo

extern "C" int mbavo_corner_score_u8(const unsigned char *d_src, int H, int W, int radius, float *d_score, void *stream)
{
    using namespace mbavo::pairs;
    if (!d_src || !d_score || radius < 1 || radius > 3 || H < 3 || W < 3) return MBAVO_E_ARG;
    const long long tiles = score_tiles(H, W);
    if (tiles > INT_MAX) return MBAVO_E_ARG; // (no such image: the tiles of a grid row)
    const dim3 grid((unsigned)tiles);
    hipStream_t st = (hipStream_t)stream;
    if (radius == 1) hipLaunchKernelGGL(k_corner_score<1>, grid, dim3(256), 0, st, d_src, H, W, d_score);
    else if (radius == 2) hipLaunchKernelGGL(k_corner_score<2>, grid, dim3(256), 0, st, d_src, H, W, d_score);
    else hipLaunchKernelGGL(k_corner_score<3>, grid, dim3(256), 0, st, d_src, H, W, d_score);
    return (int)hipGetLastError();
}

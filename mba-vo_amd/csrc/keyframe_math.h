// keyframe_math.h -- the device bodies of the keyframe pre-processing, each defined once and called by the per-image kernels
// (image_ops.hip, keyframe_ops.hip) and by the batched ones (pairs_prep.hip), so that both compute the same bits:
//
//   pyr_down_tile                          the 32 x 32 -> 16 x 16 -> 8 x 8 -> 4 x 4 pyramid tile of a workgroup
//   central_diff, GradPixel                one pixel's central differences and their three stored formats
//   gradient_magnitude                     the detector's response at a pixel
//   corner_score_of_sums, _tile            the other response: the weakest direction of the windowed structure tensor
//   GradientResponse, ScoreResponse        which of the two a selection reads, as a policy
//   best_pixel_in_cell, pick_at            a wave's pick in one grid cell
//   block_exclusive_scan, _rank_of_flag    the ordered compactions' prefix sums over a workgroup of 256
//   depth_of, depth_z_at                   the depth look-up in the formats the datasets store
//
// A kernel keeps its own indexing -- how it finds its image, level, cell or pair -- and calls these.
#ifndef MBAVO_KEYFRAME_MATH_H
#define MBAVO_KEYFRAME_MATH_H
#include "camera_math.h"
#include "pixel_math.h"
#include "vo_frontend.h"
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

namespace mbavo
{
    // 2 x 2 box with truncation (ImagePyramid.h:59-99: uchar(0.25f * (a + b + c + d)), which is (a + b + c + d) >> 2), up to three
    // levels below `src` in one launch: a workgroup of 256 takes the 32 x 32 tile (blockIdx.x, blockIdx.y) of the Hs x Ws source
    // down to 16 x 16, 8 x 8 and 4 x 4 through LDS -- the same integer operations per level.  d2, d3: read only where n reaches them.
    __device__ __forceinline__ void pyr_down_tile(const unsigned char *__restrict__ src, int Hs, int Ws, unsigned char *__restrict__ d1,
                                                  unsigned char *__restrict__ d2, unsigned char *__restrict__ d3, int n)
    {
        __shared__ int t1[16][17], t2[8][9];
        const int tid = threadIdx.x;
        const int H1 = Hs / 2, W1 = Ws / 2, H2 = H1 / 2, W2 = W1 / 2, H3 = H2 / 2, W3 = W2 / 2;
        {
            const int ty = tid >> 4, tx = tid & 15, h = blockIdx.y * 16 + ty, w = blockIdx.x * 16 + tx;
            int v = 0;
            if (h < H1 && w < W1)
            {
                const unsigned char *r0 = src + (size_t)(2 * h) * Ws + 2 * w, *r1 = r0 + Ws;
                v = ((int)r0[0] + (int)r0[1] + (int)r1[0] + (int)r1[1]) >> 2;
                d1[(size_t)h * W1 + w] = (unsigned char)v;
            }
            t1[ty][tx] = v;
        }
        if (n < 2) return;
        __syncthreads();
        if (tid < 64)
        {
            const int ty = tid >> 3, tx = tid & 7, h = blockIdx.y * 8 + ty, w = blockIdx.x * 8 + tx;
            const int v = (t1[2 * ty][2 * tx] + t1[2 * ty][2 * tx + 1] + t1[2 * ty + 1][2 * tx] + t1[2 * ty + 1][2 * tx + 1]) >> 2;
            if (h < H2 && w < W2) d2[(size_t)h * W2 + w] = (unsigned char)v; // (its four sources are inside level 1 whenever it is inside level 2)
            t2[ty][tx] = v;
        }
        if (n < 3) return;
        __syncthreads();
        if (tid < 16)
        {
            const int ty = tid >> 2, tx = tid & 3, h = blockIdx.y * 4 + ty, w = blockIdx.x * 4 + tx;
            const int v = (t2[2 * ty][2 * tx] + t2[2 * ty][2 * tx + 1] + t2[2 * ty + 1][2 * tx] + t2[2 * ty + 1][2 * tx + 1]) >> 2;
            if (h < H3 && w < W3) d3[(size_t)h * W3 + w] = (unsigned char)v;
        }
    }

    // right - left and bottom - top of pixel i = y * W + x (Gradient.h:16-75 without the factor 0.5); zero on the 1-px border
    __device__ __forceinline__ void central_diff(const unsigned char *__restrict__ src, int H, int W, int x, int y, size_t i, int &kx, int &ky)
    {
        kx = 0; ky = 0;
        if (x == 0 || y == 0 || x == W - 1 || y == H - 1) return;
        kx = (int)src[i + 1] - (int)src[i - 1];
        ky = (int)src[i + W] - (int)src[i - W];
    }
    // a pixel of a keyframe's gradient image in the formats of mbavo_problem.grad_fp16, from its intensity and differences:
    //   0  float pair [dx, dy] = 0.5f * (float)k, which equals 0.5f * ((float)right - (float)left): exact either way
    //   1  half pair: every value is a multiple of 0.5 in [-127.5, 127.5] -> exact
    //   2  intensity and both doubled differences in one word (pixel_math.h: pack_keyframe_word)
    template <int FORMAT> struct GradPixel
    {
        typedef unsigned type;
        static __device__ __forceinline__ unsigned of(int I, int kx, int ky)
        {
            if constexpr (FORMAT == 2)
                return pack_keyframe_word(I, kx, ky);
            else
            {
                const __half2 h = __floats2half2_rn(0.5f * (float)kx, 0.5f * (float)ky);
                return *reinterpret_cast<const unsigned *>(&h);
            }
        }
    };
    template <> struct GradPixel<0>
    {
        typedef float2 type;
        static __device__ __forceinline__ float2 of(int, int kx, int ky) { return make_float2(0.5f * (float)kx, 0.5f * (float)ky); }
    };

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

    // ---- the corner score (include/mbavo.h: mbavo_corner_score_u8, mbavo_pairs_set_detector; the reference's second detector
    // type, ENUM_SPARSE_SHI_TOMASI of FeatureDetectorSparse.cpp, scores with cv::goodFeaturesToTrack's minimum eigenvalue on the CPU).
    // For a level image I of H x W bytes, a pixel (x, y) and a radius r in {1, 2, 3}:
    //   kx, ky   are central_diff: right - left and bottom - top as integers, zero on the 1-pixel border
    //   a = sum kx^2, b = sum kx ky, c = sum ky^2 over the (2r+1) x (2r+1) window centred on the pixel; window positions outside
    //            the image contribute 0; n = (2r+1)^2 always, there is no renormalisation at the border; all three sums are exact
    //            in int (|a|, |b|, |c| <= 49 * 255^2)
    //   in double, with contraction off:
    //     tr = (double)(a + c)
    //     s  = sqrt((double)(a - c) * (double)(a - c) + 4.0 * (double)b * (double)b)   (the argument is an exact integer below 2^53)
    //     d  = tr - s, and d = 0 where d < 0
    //     score = (float)sqrt(d / (8.0 * n))
    // This is the RMS gradient along the weakest direction of the window, in grey levels per pixel -- the unit of
    // gradient_magnitude, so a threshold means the same kind of thing under both responses.  Every operation is exact or one
    // correctly rounded IEEE operation (the double sqrt and division are the IEEE ones here), so numpy gives the same bits.
    // A constant image scores 0; an image with ky = 0 everywhere (a vertical step edge) scores exactly 0 because s = a exactly; an
    // image with kx = ky everywhere scores exactly 0 because s = 2a exactly.
    __device__ __forceinline__ float corner_score_of_sums(int a, int b, int c, int n)
    {
#pragma clang fp contract(off)
        const double tr = (double)(a + c);
        const double s = sqrt((double)(a - c) * (double)(a - c) + 4.0 * (double)b * (double)b);
        double d = tr - s;
        if (d < 0.0) d = 0.0;
        return (float)sqrt(d / (8.0 * (double)n));
    }

    // The scores of the kTileH x kTileW tile at (y0, x0) of an H x W image by a workgroup of 256.  The tile and its halo of R + 1
    // pixels are staged from the byte image into LDS once; the three products are formed once per staged pixel that a window
    // can reach (central_diff's rule on the staged bytes: zero on the image's border, and zero outside the image); they are
    // summed separably in integers, rows then columns; a lane ends with two pixels of one column.  No atomics.  Every LDS access
    // walks a row with consecutive lanes (32 lanes = one row of the tile), so none conflicts.
    // R = 3: 24 x 40 bytes + 3 x 22 x 38 + 3 x 22 x 32 ints = 19 440 B (R = 2: 17 156, R = 1: 14 976): eight workgroups a CU either
    // way, which is the 32-wave cap.
    constexpr int kScoreTileW = 32, kScoreTileH = 16;
    template <int R>
    __device__ __forceinline__ void corner_score_tile(const unsigned char *__restrict__ src, int H, int W, int x0, int y0, float *__restrict__ score)
    {
        constexpr int TW = kScoreTileW, TH = kScoreTileH, PW = TW + 2 * R, PH = TH + 2 * R, BW = PW + 2, BH = PH + 2, N = (2 * R + 1) * (2 * R + 1);
        static_assert(TW == 32 && TH == 16, "a lane takes column tid & 31 of rows 2 (tid >> 5) and the next: 256 lanes");
        __shared__ unsigned char bytes[BH * BW];
        __shared__ int pxx[PH * PW], pxy[PH * PW], pyy[PH * PW];
        __shared__ int rxx[PH * TW], rxy[PH * TW], ryy[PH * TW];
        const int tid = threadIdx.x;
        for (int i = tid; i < BH * BW; i += 256)
        { // staged (sy, sx) is the image's (y0 - R - 1 + sy, x0 - R - 1 + sx)
            const int sy = i / BW, sx = i - sy * BW, gy = y0 - R - 1 + sy, gx = x0 - R - 1 + sx;
            bytes[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? src[(size_t)gy * W + gx] : (unsigned char)0;
        }
        __syncthreads();
        for (int i = tid; i < PH * PW; i += 256)
        { // product (py, px) is the image's (y0 - R + py, x0 - R + px) = staged (py + 1, px + 1); its four neighbours are staged
            const int py = i / PW, px = i - py * PW, gy = y0 - R + py, gx = x0 - R + px;
            int kx = 0, ky = 0;
            if (gx > 0 && gy > 0 && gx < W - 1 && gy < H - 1)
            {
                const int s = (py + 1) * BW + px + 1;
                kx = (int)bytes[s + 1] - (int)bytes[s - 1];
                ky = (int)bytes[s + BW] - (int)bytes[s - BW];
            }
            pxx[i] = kx * kx; pxy[i] = kx * ky; pyy[i] = ky * ky;
        }
        __syncthreads();
        for (int i = tid; i < PH * TW; i += 256)
        { // row sum (py, x): products (py, x .. x + 2R), the window's row around tile column x
            const int py = i / TW, x = i - py * TW, p = py * PW + x;
            int sa = 0, sb = 0, sc = 0;
#pragma unroll
            for (int j = 0; j <= 2 * R; ++j) { sa += pxx[p + j]; sb += pxy[p + j]; sc += pyy[p + j]; }
            rxx[i] = sa; rxy[i] = sb; ryy[i] = sc;
        }
        __syncthreads();
        { // tile pixel (y, x): row sums (y .. y + 2R, x); the two pixels of a lane share 2R of their rows
            const int x = tid & 31, y = 2 * (tid >> 5), q = y * TW + x;
            int a0 = 0, b0 = 0, c0 = 0;
#pragma unroll
            for (int k = 1; k <= 2 * R; ++k) { a0 += rxx[q + k * TW]; b0 += rxy[q + k * TW]; c0 += ryy[q + k * TW]; }
            const int a1 = a0 + rxx[q + (2 * R + 1) * TW], b1 = b0 + rxy[q + (2 * R + 1) * TW], c1 = c0 + ryy[q + (2 * R + 1) * TW];
            a0 += rxx[q]; b0 += rxy[q]; c0 += ryy[q];
            const int gx = x0 + x, gy = y0 + y;
            if (gx < W && gy < H) score[(size_t)gy * W + gx] = corner_score_of_sums(a0, b0, c0, N);
            if (gx < W && gy + 1 < H) score[(size_t)(gy + 1) * W + gx] = corner_score_of_sums(a1, b1, c1, N);
        }
    }

    // The response a selection reads at pixel (x, y), as a policy of best_pixel_in_cell and of the every-candidate predicate:
    // the gradient magnitude from the byte image, or the float at the pixel's index of the level's score slice.
    struct GradientResponse
    {
        __device__ __forceinline__ float at(const unsigned char *__restrict__ src, int H, int W, int x, int y) const
        {
            return gradient_magnitude(src, H, W, x, y);
        }
    };
    struct ScoreResponse
    {
        const float *score; // H * W
        __device__ __forceinline__ float at(const unsigned char *__restrict__, int, int W, int x, int y) const { return score[(size_t)y * W + x]; }
    };

    // Grid selection (FeatureDetectorBase.cpp:49-91): a wave scans the cell_h x cell_w cell at (y0, x0) of an H x W image for its
    // first pixel, in row-major order, of strictly largest response above thr; every lane ends with the same best and best_idx
    // (y * W + x; 0x7fffffff: none).
    template <class RESP>
    __device__ __forceinline__ void best_pixel_in_cell(const RESP &resp, const unsigned char *__restrict__ src, int H, int W, int y0, int x0, int cell_h,
                                                       int cell_w, float thr, int lane, float &best, int &best_idx)
    {
        best = 0.f; // cv::KeyPoint() has response 0: a pixel must beat it strictly
        best_idx = 0x7fffffff;
        const int n = cell_h * cell_w;
        for (int i = lane; i < n; i += 64)
        {
            const int y = y0 + i / cell_w, x = x0 + i % cell_w;
            if (y >= H || x >= W) continue;
            const float m = resp.at(src, H, W, x, y);
            const bool better = m > thr && best < m; // per lane the scan order is increasing
            best = better ? m : best;
            best_idx = better ? y * W + x : best_idx;
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1)
        {
            const float om = __shfl_xor(best, off);
            const int oi = __shfl_xor(best_idx, off);
            if (om > best || (om == best && oi < best_idx)) { best = om; best_idx = oi; }
        }
    }
    __device__ __forceinline__ void best_pixel_in_cell(const unsigned char *__restrict__ src, int H, int W, int y0, int x0, int cell_h, int cell_w,
                                                       float thr, int lane, float &best, int &best_idx)
    { // (by gradient magnitude)
        best_pixel_in_cell(GradientResponse{}, src, H, W, y0, x0, cell_h, cell_w, thr, lane, best, best_idx);
    }
    // the cell's pick before its depth test: keep = the cell has such a pixel (FeatureDetectorBase.cpp:82-85), x and y = where
    __device__ __forceinline__ CellPick pick_at(float best, int best_idx, int W)
    {
        CellPick p;
        p.keep = 0; p.x = 0; p.y = 0; p.z = 0.f;
        if (!(best < 1e-6))
        {
            p.y = best_idx / W; p.x = best_idx - p.y * W;
            p.keep = 1;
        }
        return p;
    }

    // ---- prefix sums over a workgroup of 256 lanes (four waves), for ordered compactions that walk their input in chunks of 256
    // with a running base.  Both return the lane's exclusive prefix within the chunk and set `total` to the chunk's sum;
    // wave_total is the caller's __shared__ int[4], and the caller's loop puts a barrier before the next chunk rewrites it.
    __device__ __forceinline__ int block_prefix_of_waves(int in_wave, int *wave_total, int &total)
    {
        const int wave = threadIdx.x >> 6;
        __syncthreads();
        int before = 0;
        total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w)
        {
            const int t = wave_total[w];
            before += w < wave ? t : 0;
            total += t;
        }
        return before + in_wave;
    }
    // of a value per lane: a shuffle scan within every wave, the four wave totals meet in LDS
    __device__ __forceinline__ int block_exclusive_scan(int v0, int *wave_total, int &total)
    {
        const int lane = threadIdx.x & 63;
        int v = v0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1)
        {
            const int t = __shfl_up(v, off);
            if (lane >= off) v += t;
        }
        if (lane == 63) wave_total[threadIdx.x >> 6] = v;
        return block_prefix_of_waves(v - v0, wave_total, total);
    }
    // of a flag per lane: the number of set flags in earlier lanes, by a ballot per wave
    __device__ __forceinline__ int block_rank_of_flag(bool flag, int *wave_total, int &total)
    {
        const int lane = threadIdx.x & 63;
        const unsigned long long b = __ballot(flag);
        if (lane == 0) wave_total[threadIdx.x >> 6] = __popcll(b);
        return block_prefix_of_waves(__popcll(b & ((1ull << lane) - 1ull)), wave_total, total);
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

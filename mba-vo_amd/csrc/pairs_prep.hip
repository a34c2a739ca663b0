// pairs_prep.hip -- the input side of a batch of keyframe pairs (include/mbavo.h: mbavo_pairs_*).
//
// What mbavo_pyramid_levels_u8, mbavo_image_gradients_u8 (_half, mbavo_pack_keyframe_u8) and mbavo_detect_semidense do for one
// image and one level per call (image_ops.hip, keyframe_ops.hip), for B pairs x L levels in ceil((L-1)/3) + 3 launches and one
// stream synchronisation, whatever B is:
//
//   pyramids         ImagePyramid.h:59-99                     2 x 2 box with truncation, three levels per launch through LDS,
//                                                             all 2B images (image index in blockIdx.z)
//   gradients        Gradient.h:16-75                         central differences of all B x L keyframe levels, 16 bytes per lane
//   grid selection   FeatureDetectorSemiDense.cpp:27-43,      one wave per cell, all B x L levels; depth test against the pair's
//                    FeatureDetectorBase.cpp:49-91,           own level-0 depth map and border test on the device
//                    blur_aware_direct_tracker.cpp:389-415
//   depth formats    blur_aware_direct_tracker.cpp:368-386    (mbavo_pairs_opts.depth_format) float z, ray distance or uint16: the
//                                                             kernels that look depths up are compiled per format and convert
//                                                             the pixels they read (keyframe_math.h: depth_z_at)
//   compaction                                                one workgroup per (pair, level): kept picks in row-major cell order
//   every candidate  FeatureDetectorSemiDense.cpp:27-43       (mbavo_pairs_opts.every_candidate, in place of the two above) no grid:
//                    without gridSelection                    count, scan, write over 256-pixel segments, one launch more
//
// The per-pixel detector functions are the per-image kernels' own (keyframe_math.h); the cell scan, the pyramid tile and the
// gradient arithmetic follow keyframe_ops.hip / image_ops.hip operation by operation: results are bit-identical to the per-image
// entry points (tests/test_gpu_pairs_prep.py holds every array to them).  The (pair, level) parameters live in a device-resident
// table written once at creation; a workgroup finds its entry from the grid index.  All streaming work, HBM-bound.
#include "pairs_prep.h"
#include "keyframe_math.h"
#include "pixel_math.h"
#include "pose_math.h"
#include "se3_math.h"
#include "vo_frontend.h"
#include <cmath>
#include <cstring>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

namespace mbavo
{
    struct PairLevelDesc
    {
        unsigned char *ref, *cur; // this level of the keyframe / the current frame
        void *grad;               // float2 / __half2 / packed word per pixel
        double *kp_xy, *kp_z;
        union
        {
            CellPick *picks;      // grid selection: `cells` of them
            int *seg;             // every candidate: one int per 256 pixels (candidate count, then its exclusive scan)
        };
        int H, W, ch, cw, cells_w, cells, border;
        double scale;             // 2^level
    };
    // where the levels start in the grids that run over all levels of a pair (by value: L <= 8)
    struct PairsGrid
    {
        int L, B;
        int blk0[9];  // gradients: first workgroup of every level
        int cell0[9]; // grid selection: first cell of every level; every candidate: first workgroup (1024 pixels) of every level
    };

    namespace pairs
    {
        constexpr long long kAlign = 256;
        // largest level-0 image: one row of the strided level-0 copy is a whole image (tested at this size)
        constexpr long long kMaxPixels = 1ll << 22;
        inline long long align_up(long long v, long long a) { return (v + a - 1) / a * a; }

        // ---- pyramids: k_pyr_down_multi (keyframe_ops.hip) over 2B images; image z < B is pair z's keyframe, else pair (z - B)'s
        // current frame; levels l0 + 1 .. l0 + n below level l0
        __device__ __forceinline__ void pyr_down_image(const PairLevelDesc *d, const bool key, const int n)
        {
            __shared__ int t1[16][17], t2[8][9];
            const int tid = threadIdx.x;
            const unsigned char *__restrict__ src = key ? d[0].ref : d[0].cur;
            unsigned char *__restrict__ d1 = key ? d[1].ref : d[1].cur;
            const int Hs = d[0].H, Ws = d[0].W;
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
                unsigned char *__restrict__ d2 = key ? d[2].ref : d[2].cur;
                const int ty = tid >> 3, tx = tid & 7, h = blockIdx.y * 8 + ty, w = blockIdx.x * 8 + tx;
                const int v = (t1[2 * ty][2 * tx] + t1[2 * ty][2 * tx + 1] + t1[2 * ty + 1][2 * tx] + t1[2 * ty + 1][2 * tx + 1]) >> 2;
                if (h < H2 && w < W2) d2[(size_t)h * W2 + w] = (unsigned char)v; // (its four sources are inside level 1 whenever it is inside level 2)
                t2[ty][tx] = v;
            }
            if (n < 3) return;
            __syncthreads();
            if (tid < 16)
            {
                unsigned char *__restrict__ d3 = key ? d[3].ref : d[3].cur;
                const int ty = tid >> 2, tx = tid & 3, h = blockIdx.y * 4 + ty, w = blockIdx.x * 4 + tx;
                const int v = (t2[2 * ty][2 * tx] + t2[2 * ty][2 * tx + 1] + t2[2 * ty + 1][2 * tx] + t2[2 * ty + 1][2 * tx + 1]) >> 2;
                if (h < H3 && w < W3) d3[(size_t)h * W3 + w] = (unsigned char)v;
            }
        }
        __global__ __launch_bounds__(256) void k_pairs_pyr_down(const PairLevelDesc *__restrict__ desc, int B, int L, int l0, int n)
        {
            const int z = blockIdx.z;
            pyr_down_image(desc + (size_t)(z < B ? z : z - B) * L + l0, z < B, n);
        }
        // (update) the images that changed: image z < n_key is the keyframe of pair key_pairs[z], else pair (z - n_key)'s current frame
        __global__ __launch_bounds__(256) void k_pairs_pyr_down_listed(const PairLevelDesc *__restrict__ desc, const int *__restrict__ key_pairs,
                                                                       int n_key, int L, int l0, int n)
        {
            const int z = blockIdx.z;
            pyr_down_image(desc + (size_t)(z < n_key ? key_pairs[z] : z - n_key) * L + l0, z < n_key, n);
        }

        // ---- gradients of all B x L keyframe levels.  A level is walked as a flat array of H*W pixels so that every lane stores 16
        // aligned bytes whatever the row length (odd widths included): 2 pixels of float pairs, 4 pixels of half pairs or packed
        // words.  The level's slice is padded to 16 pixels, so the last lane's store stays inside it (zeros in the pad).
        template <int FORMAT> struct GradOut;
        template <> struct GradOut<0>
        {
            static constexpr int kPixels = 2;
            float4 v;
            __device__ __forceinline__ void set(int j, int I, int kx, int ky)
            { // k_gradients: 0.5f * ((float)right - (float)left) == 0.5f * (float)(right - left), exact either way
                (&v.x)[2 * j] = 0.5f * (float)kx; (&v.x)[2 * j + 1] = 0.5f * (float)ky;
            }
        };
        template <> struct GradOut<1>
        {
            static constexpr int kPixels = 4;
            uint4 v;
            __device__ __forceinline__ void set(int j, int I, int kx, int ky)
            { // k_gradients_half
                const __half2 h = __floats2half2_rn(0.5f * (float)kx, 0.5f * (float)ky);
                (&v.x)[j] = *reinterpret_cast<const unsigned *>(&h);
            }
        };
        template <> struct GradOut<2>
        {
            static constexpr int kPixels = 4;
            uint4 v;
            __device__ __forceinline__ void set(int j, int I, int kx, int ky) { (&v.x)[j] = pack_keyframe_word(I, kx, ky); } // k_pack_keyframe
        };

        template <int FORMAT>
        __device__ __forceinline__ void gradients_of_pair(const PairLevelDesc *__restrict__ desc, const PairsGrid &g, const int pair)
        {
            constexpr int PPL = GradOut<FORMAT>::kPixels;
            int l = 0;
            while (l + 1 < g.L && (int)blockIdx.x >= g.blk0[l + 1]) ++l;
            const PairLevelDesc &d = desc[(size_t)pair * g.L + l];
            const int H = d.H, W = d.W, npx = H * W;
            const int i0 = (((int)blockIdx.x - g.blk0[l]) * 256 + (int)threadIdx.x) * PPL;
            if (i0 >= npx) return;
            const unsigned char *__restrict__ src = d.ref;
            int y = i0 / W, x = i0 - y * W;
            GradOut<FORMAT> out;
#pragma unroll
            for (int j = 0; j < PPL; ++j)
            {
                const int i = i0 + j;
                int I = 0, kx = 0, ky = 0;
                if (i < npx)
                {
                    I = (int)src[i];
                    if (!(x == 0 || y == 0 || x == W - 1 || y == H - 1))
                    {
                        kx = (int)src[i + 1] - (int)src[i - 1];
                        ky = (int)src[i + W] - (int)src[i - W];
                    }
                }
                out.set(j, I, kx, ky);
                if (++x == W) { x = 0; ++y; }
            }
            *reinterpret_cast<decltype(out.v) *>((char *)d.grad + (size_t)i0 * (16 / PPL)) = out.v;
        }
        template <int FORMAT>
        __global__ __launch_bounds__(256) void k_pairs_gradients(const PairLevelDesc *__restrict__ desc, const PairsGrid g)
        {
            gradients_of_pair<FORMAT>(desc, g, (int)blockIdx.y);
        }
        template <int FORMAT> // (update) grid (.., n_key): row y is pair key_pairs[y]
        __global__ __launch_bounds__(256) void k_pairs_gradients_listed(const PairLevelDesc *__restrict__ desc, const PairsGrid g,
                                                                        const int *__restrict__ key_pairs)
        {
            gradients_of_pair<FORMAT>(desc, g, key_pairs[blockIdx.y]);
        }

        // ---- grid selection: detect_cell of keyframe_ops.hip (same per-pixel functions, keyframe_math.h) with the border test
        // one wave per cell, four cells per workgroup; grid (ceil(cells of a pair / 4), B)
        // (`pair`: whose levels; the depth map is row blockIdx.y of depth_all -- the same thing in a prepare, the pair's place in the
        // list in an update -- in the element size of the depth format DF: keyframe_math.h)
        template <int DF>
        __device__ __forceinline__ const typename DepthMap<DF>::elem *depth_row(const void *__restrict__ depth_all, int H0, int W0)
        {
            return static_cast<const typename DepthMap<DF>::elem *>(depth_all) + (size_t)blockIdx.y * H0 * W0;
        }
        template <int DF>
        __device__ __forceinline__ void detect_cell_of_pair(const PairLevelDesc *__restrict__ desc, const PairsGrid &g, const int pair, float thr,
                                                            const void *__restrict__ depth_all, int H0, int W0, const DepthConv &dc)
        {
            const int lane = threadIdx.x & 63, cell = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
            if (cell >= g.cell0[g.L]) return; // (whole waves)
            int l = 0;
            while (l + 1 < g.L && cell >= g.cell0[l + 1]) ++l;
            const PairLevelDesc &d = desc[(size_t)pair * g.L + l];
            const unsigned char *__restrict__ src = d.ref;
            const int H = d.H, W = d.W, cell_h = d.ch, cell_w = d.cw, ci = cell - g.cell0[l];
            const int y0 = (ci / d.cells_w) * cell_h, x0 = (ci % d.cells_w) * cell_w;
            float best = 0.f; // cv::KeyPoint() has response 0: a pixel must beat it strictly
            int best_idx = 0x7fffffff;
            const int n = cell_h * cell_w;
            for (int i = lane; i < n; i += 64)
            {
                const int y = y0 + i / cell_w, x = x0 + i % cell_w;
                if (y >= H || x >= W) continue;
                const float m = gradient_magnitude(src, H, W, x, y);
                if (m > thr && best < m) { best = m; best_idx = y * W + x; } // per lane the scan order is increasing
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1)
            {
                const float om = __shfl_xor(best, off);
                const int oi = __shfl_xor(best_idx, off);
                if (om > best || (om == best && oi < best_idx)) { best = om; best_idx = oi; }
            }
            if (lane == 0)
            {
                CellPick p;
                p.keep = 0; p.x = 0; p.y = 0; p.z = 0.f;
                if (!(best < 1e-6)) // FeatureDetectorBase.cpp:82-85
                {
                    p.y = best_idx / W; p.x = best_idx - p.y * W;
                    const typename DepthMap<DF>::elem *depth = depth_row<DF>(depth_all, H0, W0); // the pair's own map
                    const int m = d.border;
                    const bool inside = p.x >= m && p.x < W - m && p.y >= m && p.y < H - m;
                    p.keep = (depth_of<DF>(depth, W0, d.scale, p.x, p.y, dc, p.z) && inside) ? 1 : 0;
                }
                d.picks[ci] = p;
            }
        }
        // (the conversion's constants come last: a float z map does not read them, and the arguments before them stay where they were)
        template <int DF>
        __global__ __launch_bounds__(256) void k_pairs_detect(const PairLevelDesc *__restrict__ desc, const PairsGrid g, float thr,
                                                              const void *__restrict__ depth_all, int H0, int W0, const DepthConv dc)
        {
            detect_cell_of_pair<DF>(desc, g, (int)blockIdx.y, thr, depth_all, H0, W0, dc);
        }
        template <int DF>
        __global__ __launch_bounds__(256) void k_pairs_detect_listed(const PairLevelDesc *__restrict__ desc, const PairsGrid g, float thr,
                                                                     const void *__restrict__ depth_all, int H0, int W0,
                                                                     const int *__restrict__ key_pairs, const DepthConv dc)
        {
            detect_cell_of_pair<DF>(desc, g, key_pairs[blockIdx.y], thr, depth_all, H0, W0, dc);
        }

        // ---- ordered compaction: one workgroup per (pair, level), grid (L, B).  256 cells per step: every wave ballots its 64
        // cells, the four wave totals meet in LDS, a kept pick's place is (kept so far) + (earlier waves) + (earlier lanes).
        __device__ __forceinline__ void compact_entry(const PairLevelDesc *__restrict__ desc, int *__restrict__ counts, const int e)
        {
            __shared__ int wave_total[4];
            const PairLevelDesc &d = desc[e];
            const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = d.cells;
            int base = 0;
            for (int c0 = 0; c0 < n; c0 += 256)
            {
                const int i = c0 + (int)threadIdx.x;
                CellPick p;
                p.keep = 0; p.x = 0; p.y = 0; p.z = 0.f;
                if (i < n) p = d.picks[i];
                const unsigned long long b = __ballot(p.keep != 0);
                if (lane == 0) wave_total[wave] = __popcll(b);
                __syncthreads();
                int before = 0, total = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w)
                {
                    const int v = wave_total[w];
                    before += w < wave ? v : 0;
                    total += v;
                }
                if (p.keep)
                {
                    const int pos = base + before + __popcll(b & ((1ull << lane) - 1ull)); // < cells: one pick per cell at most
                    reinterpret_cast<double2 *>(d.kp_xy)[pos] = make_double2((double)p.x, (double)p.y);
                    d.kp_z[pos] = (double)p.z;
                }
                base += total;
                __syncthreads(); // (wave_total is rewritten in the next step)
            }
            if (threadIdx.x == 0) counts[e] = base;
        }
        __global__ __launch_bounds__(256) void k_pairs_compact(const PairLevelDesc *__restrict__ desc, int *__restrict__ counts)
        {
            compact_entry(desc, counts, (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x);
        }
        __global__ __launch_bounds__(256) void k_pairs_compact_listed(const PairLevelDesc *__restrict__ desc, int *__restrict__ counts,
                                                                      const int *__restrict__ key_pairs)
        { // grid (L, n_key)
            compact_entry(desc, counts, key_pairs[blockIdx.y] * (int)gridDim.x + (int)blockIdx.x);
        }

        // ---- every candidate (mbavo_pairs_opts.every_candidate): row_candidate of keyframe_ops.hip with the border test, all
        // B x L levels in three launches.  A level is walked as a flat array of H*W pixels in segments of 256: a wave owns one
        // segment (four steps of 64 pixels, so its candidates are contiguous in row-major order), a workgroup four of them; the
        // workgroups of a pair's levels lie side by side in blockIdx.x (PairsGrid::cell0).  Count, scan, write: the order comes
        // from the scan alone -- no workgroup waits on another and nothing is atomic, so the result is deterministic.
        constexpr int kSegPixels = 256, kSegsPerGroup = 4;
        template <int DF>
        __device__ __forceinline__ bool dense_candidate(const PairLevelDesc &d, float thr, const typename DepthMap<DF>::elem *__restrict__ depth, int W0,
                                                        const DepthConv &dc, int i, int &x, int &y, float &z)
        {
            if (i >= d.H * d.W) return false;
            y = i / d.W; x = i - y * d.W;
            const int m = d.border;
            if (!(x >= m && x < d.W - m && y >= m && y < d.H - m)) return false;
            const float g = gradient_magnitude(d.ref, d.H, d.W, x, y);
            if (!(g > thr)) return false;
            return depth_of<DF>(depth, W0, d.scale, x, y, dc, z); // (x < W_l = W0 >> l: its level-0 position is inside the map)
        }
        // the wave's level and segment; false (for the whole wave) behind the level's last segment
        __device__ __forceinline__ bool dense_segment(const PairLevelDesc *__restrict__ desc, const PairsGrid &g, const int pair,
                                                      const PairLevelDesc *&d, int &seg)
        {
            int l = 0;
            while (l + 1 < g.L && (int)blockIdx.x >= g.cell0[l + 1]) ++l;
            d = desc + (size_t)pair * g.L + l;
            seg = ((int)blockIdx.x - g.cell0[l]) * kSegsPerGroup + ((int)threadIdx.x >> 6);
            return seg < (d->H * d->W + kSegPixels - 1) / kSegPixels;
        }
        template <int DF>
        __device__ __forceinline__ void dense_count_of_pair(const PairLevelDesc *__restrict__ desc, const PairsGrid &g, const int pair, float thr,
                                                            const void *__restrict__ depth_all, int H0, int W0, const DepthConv &dc)
        {
            const PairLevelDesc *d;
            int seg;
            if (!dense_segment(desc, g, pair, d, seg)) return;
            const typename DepthMap<DF>::elem *depth = depth_row<DF>(depth_all, H0, W0); // the pair's own map (as detect_cell_of_pair)
            const int lane = threadIdx.x & 63;
            int n = 0;
#pragma unroll
            for (int s = 0; s < kSegPixels / 64; ++s)
            {
                int x, y;
                float z;
                n += __popcll(__ballot(dense_candidate<DF>(*d, thr, depth, W0, dc, seg * kSegPixels + s * 64 + lane, x, y, z)));
            }
            if (lane == 0) d->seg[seg] = n;
        }
        template <int DF>
        __global__ __launch_bounds__(256) void k_pairs_dense_count(const PairLevelDesc *__restrict__ desc, const PairsGrid g, float thr,
                                                                   const void *__restrict__ depth_all, int H0, int W0, const DepthConv dc)
        {
            dense_count_of_pair<DF>(desc, g, (int)blockIdx.y, thr, depth_all, H0, W0, dc);
        }
        template <int DF>
        __global__ __launch_bounds__(256) void k_pairs_dense_count_listed(const PairLevelDesc *__restrict__ desc, const PairsGrid g, float thr,
                                                                          const void *__restrict__ depth_all, int H0, int W0,
                                                                          const int *__restrict__ key_pairs, const DepthConv dc)
        {
            dense_count_of_pair<DF>(desc, g, key_pairs[blockIdx.y], thr, depth_all, H0, W0, dc);
        }

        // in-place exclusive scan of an entry's segment counts, one workgroup per (pair, level), grid (L, B); 256 segments per
        // step: a shuffle scan within every wave, the four wave totals meet in LDS.  The total is the entry's K.
        __device__ __forceinline__ void dense_scan_entry(const PairLevelDesc *__restrict__ desc, int *__restrict__ counts, const int e)
        {
            __shared__ int wave_total[4];
            const PairLevelDesc &d = desc[e];
            const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = (d.H * d.W + kSegPixels - 1) / kSegPixels;
            int *__restrict__ seg = d.seg;
            int base = 0;
            for (int c0 = 0; c0 < n; c0 += 256)
            {
                const int i = c0 + (int)threadIdx.x;
                const int v0 = i < n ? seg[i] : 0;
                int v = v0;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1)
                {
                    const int t = __shfl_up(v, off);
                    if (lane >= off) v += t;
                }
                if (lane == 63) wave_total[wave] = v;
                __syncthreads();
                int before = 0, total = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w)
                {
                    const int t = wave_total[w];
                    before += w < wave ? t : 0;
                    total += t;
                }
                if (i < n) seg[i] = base + before + v - v0;
                base += total;
                __syncthreads(); // (wave_total is rewritten in the next step)
            }
            if (threadIdx.x == 0) counts[e] = base;
        }
        __global__ __launch_bounds__(256) void k_pairs_dense_scan(const PairLevelDesc *__restrict__ desc, int *__restrict__ counts)
        {
            dense_scan_entry(desc, counts, (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x);
        }
        __global__ __launch_bounds__(256) void k_pairs_dense_scan_listed(const PairLevelDesc *__restrict__ desc, int *__restrict__ counts,
                                                                         const int *__restrict__ key_pairs)
        { // grid (L, n_key)
            dense_scan_entry(desc, counts, key_pairs[blockIdx.y] * (int)gridDim.x + (int)blockIdx.x);
        }

        // the predicate again, the same bits; a candidate's place is (candidates before its segment) + (earlier steps of the wave)
        // + (earlier lanes): < K <= H*W, the entry's capacity
        template <int DF>
        __device__ __forceinline__ void dense_write_of_pair(const PairLevelDesc *__restrict__ desc, const PairsGrid &g, const int pair, float thr,
                                                            const void *__restrict__ depth_all, int H0, int W0, const DepthConv &dc)
        {
            const PairLevelDesc *d;
            int seg;
            if (!dense_segment(desc, g, pair, d, seg)) return;
            const typename DepthMap<DF>::elem *depth = depth_row<DF>(depth_all, H0, W0);
            const int lane = threadIdx.x & 63;
            double2 *__restrict__ kp_xy = reinterpret_cast<double2 *>(d->kp_xy);
            double *__restrict__ kp_z = d->kp_z;
            int pos = d->seg[seg];
#pragma unroll
            for (int s = 0; s < kSegPixels / 64; ++s)
            {
                int x = 0, y = 0;
                float z = 0.f;
                const bool c = dense_candidate<DF>(*d, thr, depth, W0, dc, seg * kSegPixels + s * 64 + lane, x, y, z);
                const unsigned long long b = __ballot(c);
                if (c)
                {
                    const int mine = pos + __popcll(b & ((1ull << lane) - 1ull));
                    kp_xy[mine] = make_double2((double)x, (double)y);
                    kp_z[mine] = (double)z;
                }
                pos += __popcll(b);
            }
        }
        template <int DF>
        __global__ __launch_bounds__(256) void k_pairs_dense_write(const PairLevelDesc *__restrict__ desc, const PairsGrid g, float thr,
                                                                   const void *__restrict__ depth_all, int H0, int W0, const DepthConv dc)
        {
            dense_write_of_pair<DF>(desc, g, (int)blockIdx.y, thr, depth_all, H0, W0, dc);
        }
        template <int DF>
        __global__ __launch_bounds__(256) void k_pairs_dense_write_listed(const PairLevelDesc *__restrict__ desc, const PairsGrid g, float thr,
                                                                          const void *__restrict__ depth_all, int H0, int W0,
                                                                          const int *__restrict__ key_pairs, const DepthConv dc)
        {
            dense_write_of_pair<DF>(desc, g, key_pairs[blockIdx.y], thr, depth_all, H0, W0, dc);
        }

        // ---- (update) level 0 of the new keyframes into the listed pairs' own storage: image y of src_all -> pair key_pairs[y].
        // 16 destination bytes per lane (the destination is 256-byte aligned; a source image starts wherever y * npx falls).
        __global__ __launch_bounds__(256) void k_pairs_scatter_level0(const PairLevelDesc *__restrict__ desc, int L, const int *__restrict__ key_pairs,
                                                                      const unsigned char *__restrict__ src_all, int npx)
        {
            const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 16;
            if (i0 >= npx) return;
            const unsigned char *__restrict__ src = src_all + (size_t)blockIdx.y * npx + i0;
            unsigned char *__restrict__ dst = desc[(size_t)key_pairs[blockIdx.y] * L].ref + i0;
            if (i0 + 16 <= npx && ((size_t)src & 3) == 0)
            {
                const unsigned *s4 = reinterpret_cast<const unsigned *>(src);
                *reinterpret_cast<uint4 *>(dst) = make_uint4(s4[0], s4[1], s4[2], s4[3]);
            }
            else
                for (int j = 0; j < 16 && i0 + j < npx; ++j) dst[j] = src[j];
        }

        // ---- the keyframe test and the frame pose of every pair (vo_frontend.cpp: BlurAwareDirectTracker::isKeyframe,
        // blur_aware_direct_tracker.cpp:205-262): one workgroup per pair.  Lanes 0..2 sample the pair's spline at the capture time
        // and at -/+ half the exposure (SplineSE3::GetPose) and invert the poses (Core::Transformation::inverse) into LDS; every
        // lane then strides over the level-0 keypoints with the host loop's arithmetic, operation for operation (no contraction:
        // the host build has no FMA), and keeps two double sums.  The sums meet in a fixed order -- butterfly within the wave, then
        // the four waves in wave order -- so the result has the same bits whatever B is and wherever the workgroup ran.
        struct AssessArgs
        {
            const PairLevelDesc *desc;
            const int *counts;
            const double *cap, *exp, *kt, *kR, *t0;
            double dt, K[4], flow_mag0, flow_mag1, max_blur_kernel_mag;
            int L, N;
            mbavo_pairs_assessment *out;
        };

        template <int KDEG>
        __device__ bool spline_pose(const double *__restrict__ kt, const double *__restrict__ kR, int N, double t0, double dt, double t, Quat &q, double p[3])
        { // SplineSE3::GetPose without Jacobians
            int idx;
            double u;
            spline_segment(t, t0, dt, idx, u);
            if (!(t == t) || idx < 0 || idx + KDEG > N) return false;
            double c[KDEG];
            trans_coeffs<KDEG>(u, c);
            spline_translation<KDEG>(kt + 3 * idx, c, p);
            q = spline_rotation<KDEG, false>(kR + 4 * idx, u, nullptr);
            return true;
        }

        // pair b's assessment into *out, by the whole workgroup.  Returns -1 in every lane when one of the three times lies outside
        // the knots; else the verdict in lane 0 (0 in the others), and T = the pose at the capture time (shared memory, lane 0's
        // to read).  One body for k_pairs_assess and k_pairs_commit: the same operations, the same bits.
        template <int KDEG>
        __device__ __forceinline__ int assess_pair(const AssessArgs &a, const int b, mbavo_pairs_assessment *out, const double *&T)
        {
            __shared__ double s_inv[3][7], s_T[7], s_sum[4][2];
            __shared__ int s_bad[3], s_behind[4];
            const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
            T = s_T;
            const int K = a.counts[(size_t)b * a.L]; // level 0 of the last prepare / update
            if (tid < 3)
            {
                const double cap = a.cap[b], ex = a.exp[b];
                const double t = tid == 0 ? cap : (tid == 1 ? cap - 0.5 * ex : cap + 0.5 * ex);
                Quat q;
                double p[3], T[7], Ti[7];
                const bool ok = spline_pose<KDEG>(a.kt + (size_t)b * 3 * a.N, a.kR + (size_t)b * 4 * a.N, a.N, a.t0[b], a.dt, t, q, p);
                s_bad[tid] = ok ? 0 : 1;
                if (ok)
                {
                    pose_make(q, p, T);
                    pose_inverse(T, Ti);
                    for (int i = 0; i < 7; ++i) s_inv[tid][i] = Ti[i];
                    if (tid == 0)
                    { // the pose as GetPose returns it
                        s_T[0] = p[0]; s_T[1] = p[1]; s_T[2] = p[2];
                        s_T[3] = q.x; s_T[4] = q.y; s_T[5] = q.z; s_T[6] = q.w;
                    }
                }
            }
            __syncthreads();
            if (s_bad[0] | s_bad[1] | s_bad[2])
            { // isKeyframe returns false before the loop
                if (tid == 0)
                {
                    const double nan = __builtin_nan("");
                    out->is_keyframe = 0; out->status = MBAVO_E_RANGE; out->num_keypoints0 = K; out->num_behind = 0;
                    out->avg_flow = nan; out->avg_kernel = nan;
                    for (int i = 0; i < 7; ++i) out->T[i] = nan;
                }
                return -1;
            }
            Quat qi[3];
            double ti[3][3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
            {
                ti[j][0] = s_inv[j][0]; ti[j][1] = s_inv[j][1]; ti[j][2] = s_inv[j][2];
                qi[j] = Quat{s_inv[j][3], s_inv[j][4], s_inv[j][5], s_inv[j][6]};
            }
            const double fx = a.K[0], fy = a.K[1], cx = a.K[2], cy = a.K[3];
            const PairLevelDesc &d = a.desc[(size_t)b * a.L];
            const double2 *__restrict__ kp_xy = reinterpret_cast<const double2 *>(d.kp_xy);
            const double *__restrict__ kp_z = d.kp_z;
            double flow = 0.0, kern = 0.0;
            int behind = 0;
            for (int i = tid; i < K; i += 256)
            {
#pragma clang fp contract(off)
                const double2 xy = kp_xy[i];
                const double x = xy.x, y = xy.y, z = kp_z[i];
                const double P[3] = {(x - cx) / fx * z, (y - cy) / fy * z, z};
                double pj[3][2] = {{0, 0}, {0, 0}, {0, 0}};
#pragma unroll
                for (int j = 0; j < 3; ++j)
                {
                    double Pc[3];
                    qrotate(qi[j], P, Pc);
                    Pc[0] += ti[j][0]; Pc[1] += ti[j][1]; Pc[2] += ti[j][2];
                    if (Pc[2] < 0) { ++behind; continue; }
                    pj[j][0] = fx * (Pc[0] / (Pc[2] + 1e-8)) + cx;
                    pj[j][1] = fy * (Pc[1] / (Pc[2] + 1e-8)) + cy;
                }
                flow += (pj[0][0] - x) * (pj[0][0] - x) + (pj[0][1] - y) * (pj[0][1] - y);
                kern += (pj[1][0] - pj[2][0]) * (pj[1][0] - pj[2][0]) + (pj[1][1] - pj[2][1]) * (pj[1][1] - pj[2][1]);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1)
            { // (a + b is commutative: every lane of the wave ends with the same bits)
                flow += __shfl_xor(flow, off);
                kern += __shfl_xor(kern, off);
                behind += __shfl_xor(behind, off);
            }
            if (lane == 0) { s_sum[wave][0] = flow; s_sum[wave][1] = kern; s_behind[wave] = behind; }
            __syncthreads();
            if (tid == 0)
            {
                const double sf = ((s_sum[0][0] + s_sum[1][0]) + s_sum[2][0]) + s_sum[3][0];
                const double sk = ((s_sum[0][1] + s_sum[1][1]) + s_sum[2][1]) + s_sum[3][1];
                const double avg_flow = sqrtf((float)(sf / K)), avg_kernel = sqrtf((float)(sk / K)); // (K = 0: NaN, every test below false)
                int kf = 0;
                if (avg_flow > a.flow_mag0 && avg_kernel < a.max_blur_kernel_mag) kf = 1;
                if (avg_flow > a.flow_mag1) kf = 1;
                out->is_keyframe = kf; out->status = 0; out->num_keypoints0 = K;
                out->num_behind = ((s_behind[0] + s_behind[1]) + s_behind[2]) + s_behind[3];
                out->avg_flow = avg_flow; out->avg_kernel = avg_kernel;
                for (int i = 0; i < 7; ++i) out->T[i] = s_T[i];
                return kf;
            }
            return 0;
        }
        template <int KDEG>
        __global__ __launch_bounds__(256) void k_pairs_assess(const AssessArgs a)
        {
            const double *T;
            (void)assess_pair<KDEG>(a, (int)blockIdx.x, a.out + blockIdx.x, T);
        }

        // ---- the tracker state of every pair (trackFrame's pose bookkeeping, blur_aware_direct_tracker.cpp:119-141 and 143-203),
        // kStateLen doubles per pair
        constexpr int kStateKeyframe = 0, kStatePrev = 7, kStateVelocity = 14, kStatePrevTime = 20, kStateDtFrame = 21, kStateLen = 22;
        struct TrackArgs
        {
            double *state;                 // B x kStateLen
            double *kt, *kR;               // the knots the problems point at: B x 3N, B x 4N
            double *cap, *exp, *t0;        // the motion's times, B each: what the LM kernels and the assessment read
            const double *times;           // predict: [cap | exp | t0] as uploaded
            mbavo_pairs_frame *frames;     // commit: B
            int B, N;
        };

        // The constant-velocity prediction (:119-141): 16 lanes per pair, 16 pairs per workgroup.  The first lane of a pair forms
        // dT = exp(velocity * dt_frame) once, into LDS, keeps dt_frame for the commit and publishes the frame's times; lane i then
        // moves knot i: SplineSE3::TransformByRight.  A pair touches nothing of another's: the same bits for any B.
        __global__ __launch_bounds__(256) void k_pairs_predict(const TrackArgs p)
        {
            __shared__ double s_dT[16][7];
            const int g = threadIdx.x >> 4, i = threadIdx.x & 15, b = (int)blockIdx.x * 16 + g;
            if (b < p.B && i == 0)
            {
#pragma clang fp contract(off)
                double *st = p.state + (size_t)b * kStateLen;
                const double cap = p.times[b], ex = p.times[p.B + b], t0 = p.times[2 * p.B + b];
                const double dt_frame = cap - st[kStatePrevTime];
                double v[6], dT[7];
#pragma unroll
                for (int j = 0; j < 6; ++j) v[j] = st[kStateVelocity + j] * dt_frame;
                se3_exp(v, dT);
#pragma unroll
                for (int j = 0; j < 7; ++j) s_dT[g][j] = dT[j];
                st[kStateDtFrame] = dt_frame;
                p.cap[b] = cap; p.exp[b] = ex; p.t0[b] = t0;
            }
            __syncthreads();
            if (b < p.B && i < p.N)
            {
                double *kt = p.kt + ((size_t)b * p.N + i) * 3, *kR = p.kR + ((size_t)b * p.N + i) * 4;
                const double d[3] = {s_dT[g][0], s_dT[g][1], s_dT[g][2]};
                const Quat dq{s_dT[g][3], s_dT[g][4], s_dT[g][5], s_dT[g][6]}, R = load_quat(kR);
                double r[3];
                qrotate(R, d, r);
                kt[0] += r[0]; kt[1] += r[1]; kt[2] += r[2];
                const Quat n = qmul(R, dq);
                kR[0] = n.x; kR[1] = n.y; kR[2] = n.z; kR[3] = n.w;
            }
        }

        // The assessment and the state update behind it (:143-203), a workgroup per pair: assess_pair, then lane 0 does the pose
        // algebra of the frame (velocity, T_prev, and for a new keyframe T_keyframe and TransformTo's right factor), lanes 0 .. N-1
        // re-express their knot where the verdict is "keyframe", and lane 0 samples the knots as they now are for T_world.
        template <int KDEG>
        __global__ __launch_bounds__(256) void k_pairs_commit(const AssessArgs a, const TrackArgs c)
        {
            __shared__ double s_right[7], s_kt[16 * 3], s_kR[16 * 4];
            __shared__ int s_rebase;
            const int b = blockIdx.x, tid = threadIdx.x, N = c.N;
            mbavo_pairs_frame *f = c.frames + b;
            const double *T;
            const int verdict = assess_pair<KDEG>(a, b, &f->a, T);
            if (verdict < 0)
            { // the state stays as the predict left it
                if (tid == 0)
                    for (int i = 0; i < 7; ++i) f->T_world[i] = __builtin_nan("");
                return;
            }
            double Tk[7];
            if (tid == 0)
            {
#pragma clang fp contract(off)
                double *st = c.state + (size_t)b * kStateLen;
                double Tb[7], Tp[7], Tpi[7], dTn[7], lg[6];
                pose_make(Quat{T[3], T[4], T[5], T[6]}, T, Tb); // T_b2w
#pragma unroll
                for (int i = 0; i < 7; ++i) { Tk[i] = st[kStateKeyframe + i]; Tp[i] = st[kStatePrev + i]; }
                pose_inverse(Tp, Tpi);
                pose_mul(Tpi, Tb, dTn); // :150-155
                se3_log(dTn, lg);
                const double dt_frame = st[kStateDtFrame];
#pragma unroll
                for (int i = 0; i < 6; ++i) st[kStateVelocity + i] = lg[i] / dt_frame;
                int rebase = 0;
                if (verdict)
                { // :176-188
                    double Tn[7];
                    pose_mul(Tk, Tb, Tn);
#pragma unroll
                    for (int i = 0; i < 7; ++i) { Tk[i] = Tn[i]; st[kStateKeyframe + i] = Tn[i]; Tb[i] = i == 6 ? 1.0 : 0.0; }
                    // SplineSE3::TransformTo(cap, identity) (Spline.h:183-200): dR = R(cap)^-1, dt = R(cap)^-1 * (0 - t(cap))
                    const double n2 = T[3] * T[3] + T[4] * T[4] + T[5] * T[5] + T[6] * T[6];
                    if (n2 > 0)
                    {
                        const Quat qi{-T[3] / n2, -T[4] / n2, -T[5] / n2, T[6] / n2};
                        const Quat dR = qmul(qi, Quat{0.0, 0.0, 0.0, 1.0});
                        const double d[3] = {0.0 - T[0], 0.0 - T[1], 0.0 - T[2]};
                        double dt3[3];
                        qrotate(qi, d, dt3);
                        s_right[0] = dt3[0]; s_right[1] = dt3[1]; s_right[2] = dt3[2];
                        s_right[3] = dR.x; s_right[4] = dR.y; s_right[5] = dR.z; s_right[6] = dR.w;
                        rebase = 1;
                    }
                }
#pragma unroll
                for (int i = 0; i < 7; ++i) st[kStatePrev + i] = Tb[i];
                st[kStatePrevTime] = a.cap[b];
                s_rebase = rebase;
            }
            __syncthreads();
            if (tid < N)
            {
                double *kt = c.kt + ((size_t)b * N + tid) * 3, *kR = c.kR + ((size_t)b * N + tid) * 4;
                double t[3] = {kt[0], kt[1], kt[2]};
                Quat R = load_quat(kR);
                if (s_rebase)
                { // TransformByRight
                    const double d[3] = {s_right[0], s_right[1], s_right[2]};
                    double r[3];
                    qrotate(R, d, r);
                    t[0] += r[0]; t[1] += r[1]; t[2] += r[2];
                    R = qmul(R, Quat{s_right[3], s_right[4], s_right[5], s_right[6]});
                    kt[0] = t[0]; kt[1] = t[1]; kt[2] = t[2];
                    kR[0] = R.x; kR[1] = R.y; kR[2] = R.z; kR[3] = R.w;
                }
                s_kt[3 * tid] = t[0]; s_kt[3 * tid + 1] = t[1]; s_kt[3 * tid + 2] = t[2];
                s_kR[4 * tid] = R.x; s_kR[4 * tid + 1] = R.y; s_kR[4 * tid + 2] = R.z; s_kR[4 * tid + 3] = R.w;
            }
            __syncthreads();
            if (tid == 0)
            {
                Quat q;
                double p[3], P[7], Tw[7];
                if (spline_pose<KDEG>(s_kt, s_kR, N, a.t0[b], a.dt, a.cap[b], q, p))
                {
                    pose_make(q, p, P);
                    pose_mul(Tk, P, Tw);
                }
                else // (the same time on the same segment as above: cannot fail)
                    for (int i = 0; i < 7; ++i) Tw[i] = __builtin_nan("");
                for (int i = 0; i < 7; ++i) f->T_world[i] = Tw[i];
            }
        }
    } // namespace pairs

    using namespace pairs;

    // the step's device buffer: [assessments B | key list B ints]
    static size_t step_off_keys(int B) { return (size_t)align_up((long long)sizeof(mbavo_pairs_assessment) * B, kAlign); }
    static size_t step_bytes(int B) { return step_off_keys(B) + (size_t)align_up((long long)sizeof(int) * B, kAlign); }

    // where the levels start in the kernels' grids
    static PairsGrid pairs_grid(const PairsPlan &p)
    {
        PairsGrid g;
        memset(&g, 0, sizeof(g));
        g.L = p.L; g.B = p.B;
        const int ppl = p.format == 0 ? 2 : 4;
        for (int l = 0; l < p.L; ++l)
        {
            g.blk0[l + 1] = g.blk0[l] + (p.H[l] * p.W[l] + 256 * ppl - 1) / (256 * ppl);
            g.cell0[l + 1] = p.dense ? g.cell0[l] + (p.seg0[l + 1] - p.seg0[l] + kSegsPerGroup - 1) / kSegsPerGroup : p.cell0[l + 1];
        }
        return g;
    }

    // The keypoint launches of a prepare (d_keys null: grid (.., B), row = pair) or of an update (grid (.., rows), row = the
    // pair's place in the key list), reading the depth maps in format DF; the number of launches.
    template <int DF>
    static int launch_keypoints(const PairsPlan &p, const PairsGrid &g, hipStream_t st, const PairLevelDesc *desc, int *d_counts, float thr,
                                const void *d_depth, const DepthConv &dc, int rows, const int *d_keys)
    {
        const int L = p.L, H0 = p.H[0], W0 = p.W[0];
        if (p.dense)
        { // every candidate: count, scan, write
            const dim3 grid(g.cell0[L], rows);
            if (d_keys)
            {
                hipLaunchKernelGGL(k_pairs_dense_count_listed<DF>, grid, dim3(256), 0, st, desc, g, thr, d_depth, H0, W0, d_keys, dc);
                hipLaunchKernelGGL(k_pairs_dense_scan_listed, dim3(L, rows), dim3(256), 0, st, desc, d_counts, d_keys);
                hipLaunchKernelGGL(k_pairs_dense_write_listed<DF>, grid, dim3(256), 0, st, desc, g, thr, d_depth, H0, W0, d_keys, dc);
            }
            else
            {
                hipLaunchKernelGGL(k_pairs_dense_count<DF>, grid, dim3(256), 0, st, desc, g, thr, d_depth, H0, W0, dc);
                hipLaunchKernelGGL(k_pairs_dense_scan, dim3(L, rows), dim3(256), 0, st, desc, d_counts);
                hipLaunchKernelGGL(k_pairs_dense_write<DF>, grid, dim3(256), 0, st, desc, g, thr, d_depth, H0, W0, dc);
            }
            return 3;
        }
        const dim3 grid((p.cell0[L] + 3) / 4, rows);
        if (d_keys)
        {
            hipLaunchKernelGGL(k_pairs_detect_listed<DF>, grid, dim3(256), 0, st, desc, g, thr, d_depth, H0, W0, d_keys, dc);
            hipLaunchKernelGGL(k_pairs_compact_listed, dim3(L, rows), dim3(256), 0, st, desc, d_counts, d_keys);
        }
        else
        {
            hipLaunchKernelGGL(k_pairs_detect<DF>, grid, dim3(256), 0, st, desc, g, thr, d_depth, H0, W0, dc);
            hipLaunchKernelGGL(k_pairs_compact, dim3(L, rows), dim3(256), 0, st, desc, d_counts);
        }
        return 2;
    }
    static int launch_keypoints(int depth_format, const PairsPlan &p, const PairsGrid &g, hipStream_t st, const PairLevelDesc *desc, int *d_counts,
                                float thr, const void *d_depth, const DepthConv &dc, int rows, const int *d_keys)
    {
        if (depth_format == 0) return launch_keypoints<0>(p, g, st, desc, d_counts, thr, d_depth, dc, rows, d_keys);
        if (depth_format == 1) return launch_keypoints<1>(p, g, st, desc, d_counts, thr, d_depth, dc, rows, d_keys);
        return launch_keypoints<2>(p, g, st, desc, d_counts, thr, d_depth, dc, rows, d_keys);
    }

    int pairs_plan(const mbavo_pairs_opts *o, PairsPlan &p)
    {
        if (!o) return MBAVO_E_ARG;
        memset(&p, 0, sizeof(p));
        const int B = o->B, L = o->L;
        if (B < 1 || B > 32767 || L < 1 || L > 8 || o->H < 1 || o->W < 1) return MBAVO_E_ARG;
        if ((o->H >> (L - 1)) < 8 || (o->W >> (L - 1)) < 8 || (long long)o->H * o->W > kMaxPixels) return MBAVO_E_ARG;
        if ((o->spline_deg_k != 2 && o->spline_deg_k != 4) || o->N < o->spline_deg_k || o->N > 16) return MBAVO_E_ARG;
        if (o->every_candidate != 0 && o->every_candidate != 1) return MBAVO_E_ARG;
        if (!depth_format_valid(o->depth_format, o->depth_unit)) return MBAVO_E_ARG; // (the object stores no depth map: no byte depends on it)
        const bool dense = o->every_candidate == 1; // no grid: cell_H, cell_W are not read
        if ((!dense && (o->cell_H < 1 || o->cell_W < 1)) || o->keyframe_format < 0 || o->keyframe_format > 2) return MBAVO_E_ARG;
        p.dense = dense ? 1 : 0;
        p.B = B; p.L = L; p.N = o->N; p.format = o->keyframe_format; p.grad_bytes = o->keyframe_format == 0 ? 8 : 4;
        for (int l = 0; l < L; ++l)
        {
            if (o->S[l] < 1 || o->P[l] < 1 || !o->pattern_xy[l] || o->border[l] < 0) return MBAVO_E_ARG;
            const int Hl = o->H >> l, Wl = o->W >> l;
            p.H[l] = Hl; p.W[l] = Wl;
            if (dense)
            { // every pixel may be a keypoint; one segment count per 256 pixels, no picks
                p.cap[l] = Hl * Wl;
                p.seg0[l + 1] = p.seg0[l] + (Hl * Wl + kSegPixels - 1) / kSegPixels;
                p.cell0[l + 1] = 0;
            }
            else
            {
                // FeatureDetectorBase.cpp:56-64 (as detect_semidense, keyframe_ops.hip)
                const int sf = (int)std::pow(2, l);
                const int ch = (int)(o->cell_H / std::pow(1.414, l)), cw = (int)(o->cell_W / std::pow(1.414, l));
                if (ch < 1 || cw < 1) return MBAVO_E_ARG; // the reference divides by zero here
                const int cells_h = (o->H / sf) / ch + 1, cells_w = (o->W / sf) / cw + 1;
                // (level l is (H >> l) x (W >> l) = the size the grid is made for: every pixel's cell exists, so detect_semidense's
                // MBAVO_E_RANGE -- an image larger than the grid of the H0 x W0 it is given -- cannot occur here)
                p.ch[l] = ch; p.cw[l] = cw; p.cells_w[l] = cells_w; p.cells[l] = cells_h * cells_w;
                p.cap[l] = p.cells[l];
                p.cell0[l + 1] = p.cell0[l] + p.cells[l];
            }
            p.px0[l + 1] = p.px0[l] + align_up((long long)Hl * Wl, 16);
            p.kp0[l + 1] = p.kp0[l] + 3ll * align_up(p.cap[l], 2);
            p.pat0[l + 1] = p.pat0[l] + 2 * o->P[l];
        }
        p.img_stride = align_up(p.px0[L], kAlign);
        p.grad_stride = align_up(p.px0[L] * p.grad_bytes, kAlign);
        p.kp_stride = p.kp0[L];
        long long at = 0;
        auto take = [&at](long long bytes) { const long long o_ = at; at = align_up(at + bytes, kAlign); return o_; };
        p.off_img = take(2ll * B * p.img_stride);
        p.off_grad = take((long long)B * p.grad_stride);
        p.off_kp = take((long long)B * p.kp_stride * 8);
        p.off_picks = take((long long)B * p.cell0[L] * (long long)sizeof(CellPick)); // (every candidate: nothing)
        p.off_seg = take((long long)B * p.seg0[L] * 4);                              // (grid selection: nothing)
        p.off_counts = take((long long)B * L * 4);
        p.off_desc = take((long long)B * L * (long long)sizeof(PairLevelDesc));
        p.off_cur_ptrs = take((long long)B * L * 8);
        p.off_pattern = take((long long)p.pat0[L] * 4);
        p.off_motion = take((long long)B * (2 + 7 * o->N) * 8);
        p.total = at;
        return 0;
    }

    PairBatch::~PairBatch()
    {
        if (!arena_ && !h_counts_ && !h_motion_ && !step_ && !h_assess_ && !h_keys_ && !h_state_ && !h_times_ && !h_frames_) return;
        (void)hipSetDevice(eng_.device());
        (void)hipStreamSynchronize(eng_.stream());
        if (arena_) (void)hipFree(arena_);
        if (step_) (void)hipFree(step_);
        if (h_assess_) (void)hipHostFree(h_assess_);
        if (h_keys_) (void)hipHostFree(h_keys_);
        if (h_counts_) (void)hipHostFree(h_counts_);
        if (h_motion_) (void)hipHostFree(h_motion_);
        if (h_state_) (void)hipHostFree(h_state_);
        if (h_times_) (void)hipHostFree(h_times_);
        if (h_frames_) (void)hipHostFree(h_frames_);
    }

    int PairBatch::create(const mbavo_pairs_opts *o)
    {
        int rc = pairs_plan(o, plan_);
        if (rc != 0) return rc;
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L, N = p.N;
        opts_ = *o;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        // (the tracker state sits behind the plan's arrays, in the same allocation: see pairs_prep.h)
        off_t0_ = p.total;
        off_state_ = off_t0_ + align_up((long long)sizeof(double) * B, kAlign);
        off_times_ = off_state_ + align_up((long long)sizeof(double) * kStateLen * B, kAlign);
        off_frames_ = off_times_ + align_up((long long)sizeof(double) * 3 * B, kAlign);
        arena_bytes_ = off_frames_ + align_up((long long)sizeof(mbavo_pairs_frame) * B, kAlign);
        if ((e = hipMalloc((void **)&arena_, (size_t)arena_bytes_)) != hipSuccess) { arena_ = nullptr; return (int)e; }
        if ((e = hipHostMalloc((void **)&h_counts_, sizeof(int) * B * L)) != hipSuccess) { h_counts_ = nullptr; return (int)e; }
        if ((e = hipHostMalloc((void **)&h_motion_, sizeof(double) * B * (3 + 7 * N))) != hipSuccess) { h_motion_ = nullptr; return (int)e; }
        if ((e = hipMalloc((void **)&step_, step_bytes(B))) != hipSuccess) { step_ = nullptr; return (int)e; }
        if ((e = hipHostMalloc((void **)&h_assess_, sizeof(mbavo_pairs_assessment) * B)) != hipSuccess) { h_assess_ = nullptr; return (int)e; }
        if ((e = hipHostMalloc((void **)&h_keys_, sizeof(int) * B)) != hipSuccess) { h_keys_ = nullptr; return (int)e; }
        const size_t state_bytes = (size_t)(off_times_ - (p.off_motion + (long long)sizeof(double) * 2 * B));
        if ((e = hipHostMalloc((void **)&h_state_, state_bytes)) != hipSuccess) { h_state_ = nullptr; return (int)e; }
        memset(h_state_, 0, state_bytes);
        if ((e = hipHostMalloc((void **)&h_times_, sizeof(double) * 3 * B)) != hipSuccess) { h_times_ = nullptr; return (int)e; }
        if ((e = hipHostMalloc((void **)&h_frames_, sizeof(mbavo_pairs_frame) * B)) != hipSuccess) { h_frames_ = nullptr; return (int)e; }
        hipStream_t st = eng_.stream();
        // deterministic contents for what a prepare does not write (pads) and for the motion before set_motion
        if ((e = hipMemsetAsync(arena_, 0, (size_t)arena_bytes_, st)) != hipSuccess) return (int)e;
        if ((e = hipMemsetAsync(step_, 0, step_bytes(B), st)) != hipSuccess) return (int)e;

        std::vector<PairLevelDesc> desc((size_t)B * L);
        std::vector<const unsigned char *> cur_ptrs((size_t)B * L);
        std::vector<int> pattern(p.pat0[L]);
        for (int l = 0; l < L; ++l) memcpy(&pattern[p.pat0[l]], o->pattern_xy[l], sizeof(int) * 2 * o->P[l]);
        double *motion = (double *)(arena_ + p.off_motion);
        double *d_cap = motion, *d_exp = motion + B, *d_kt = motion + 2 * B, *d_kR = d_kt + (size_t)B * 3 * N;
        probs_.assign((size_t)B * L, mbavo_problem{});
        start_idx_.assign(B, 0);
        for (int b = 0; b < B; ++b)
            for (int l = 0; l < L; ++l)
            {
                const size_t e_ = (size_t)b * L + l;
                PairLevelDesc &d = desc[e_];
                d.ref = (unsigned char *)arena_ + p.off_img + (long long)b * p.img_stride + p.px0[l];
                d.cur = (unsigned char *)arena_ + p.off_img + (long long)(B + b) * p.img_stride + p.px0[l];
                d.grad = arena_ + p.off_grad + (long long)b * p.grad_stride + p.px0[l] * p.grad_bytes;
                d.kp_xy = (double *)(arena_ + p.off_kp) + (long long)b * p.kp_stride + p.kp0[l];
                d.kp_z = d.kp_xy + 2 * align_up(p.cap[l], 2);
                if (p.dense) d.seg = (int *)(arena_ + p.off_seg) + (long long)b * p.seg0[L] + p.seg0[l];
                else d.picks = (CellPick *)(arena_ + p.off_picks) + (long long)b * p.cell0[L] + p.cell0[l];
                d.H = p.H[l]; d.W = p.W[l]; d.ch = p.ch[l]; d.cw = p.cw[l]; d.cells_w = p.cells_w[l]; d.cells = p.cells[l];
                d.border = o->border[l]; d.scale = std::pow(2, l);
                cur_ptrs[e_] = d.cur;
                mbavo_problem &q = probs_[e_];
                q.S = o->S[l]; q.F = 1; q.K = 0; q.P = o->P[l]; q.N = N; q.H = d.H; q.W = d.W;
                q.d_ref_img = d.ref; q.d_ref_dIxy = (const float *)d.grad;
                q.d_cur_imgs = (const unsigned char *const *)(arena_ + p.off_cur_ptrs) + e_;
                q.d_kp_xy = d.kp_xy; q.kp_stride = 2; q.d_kp_z = d.kp_z;
                q.d_pattern = (const int *)(arena_ + p.off_pattern) + p.pat0[l];
                q.d_outlier = nullptr; q.num_bad = 0;
                for (int a = 0; a < 4; ++a) q.intrinsics[a] = o->intrinsics[a] / (double)(1 << l);
                q.d_cap_time = d_cap + b; q.d_exp_time = d_exp + b;
                q.d_knots_t = d_kt + (size_t)b * 3 * N; q.d_knots_R = d_kR + (size_t)b * 4 * N;
                q.h_start_idx = &start_idx_[b];
                q.huber_a = o->huber_a; q.grad_fp16 = p.format;
            }
        // (pageable sources: the copies are staged before the calls return; the synchronisation below covers the rest)
        if ((e = hipMemcpyAsync(arena_ + p.off_desc, desc.data(), sizeof(PairLevelDesc) * desc.size(), hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        if ((e = hipMemcpyAsync(arena_ + p.off_cur_ptrs, cur_ptrs.data(), sizeof(void *) * cur_ptrs.size(), hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        if ((e = hipMemcpyAsync(arena_ + p.off_pattern, pattern.data(), sizeof(int) * pattern.size(), hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        return (int)hipStreamSynchronize(st);
    }

    DepthConv PairBatch::depth_conv() const
    {
        DepthConv c;
        c.fx = opts_.intrinsics[0]; c.fy = opts_.intrinsics[1]; c.cx = opts_.intrinsics[2]; c.cy = opts_.intrinsics[3];
        c.unit = opts_.depth_unit; c.max = opts_.depth_max;
        return c;
    }

    // (d_depth: B maps in the object's depth format -- float z, float ray distance or uint16)
    int PairBatch::prepare(const unsigned char *d_sharp, const void *d_depth, const unsigned char *d_blur, int *h_counts)
    {
        if (!arena_ || !d_sharp || !d_depth || !d_blur) return MBAVO_E_ARG;
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        const PairLevelDesc *desc = (const PairLevelDesc *)(arena_ + p.off_desc);
        int *d_counts = (int *)(arena_ + p.off_counts);
        stats_[0] = stats_[1] = stats_[2] = 0;
        // level 0 of both images into the object's own storage (one strided copy each)
        const size_t npx0 = (size_t)p.H[0] * p.W[0];
        unsigned char *img = (unsigned char *)arena_ + p.off_img;
        if ((e = hipMemcpy2DAsync(img, (size_t)p.img_stride, d_sharp, npx0, npx0, B, hipMemcpyDeviceToDevice, st)) != hipSuccess) return (int)e;
        if ((e = hipMemcpy2DAsync(img + (size_t)B * p.img_stride, (size_t)p.img_stride, d_blur, npx0, npx0, B, hipMemcpyDeviceToDevice, st)) != hipSuccess)
            return (int)e;
        const PairsGrid g = pairs_grid(p);
        for (int l = 0; l + 1 < L; l += 3)
        {
            const int n = L - 1 - l < 3 ? L - 1 - l : 3;
            hipLaunchKernelGGL(k_pairs_pyr_down, dim3((p.W[l] / 2 + 15) / 16, (p.H[l] / 2 + 15) / 16, 2 * B), dim3(256), 0, st, desc, B, L, l, n);
            ++stats_[0];
        }
        const dim3 ggrid(g.blk0[L], B);
        if (p.format == 0) hipLaunchKernelGGL(k_pairs_gradients<0>, ggrid, dim3(256), 0, st, desc, g);
        else if (p.format == 1) hipLaunchKernelGGL(k_pairs_gradients<1>, ggrid, dim3(256), 0, st, desc, g);
        else hipLaunchKernelGGL(k_pairs_gradients<2>, ggrid, dim3(256), 0, st, desc, g);
        stats_[0] += 1 + launch_keypoints(opts_.depth_format, p, g, st, desc, d_counts, opts_.score_threshold, d_depth, depth_conv(), B, nullptr);
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        if ((e = hipMemcpyAsync(h_counts_, d_counts, sizeof(int) * B * L, hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
        stats_[2] = (long long)sizeof(int) * B * L;
        e = hipStreamSynchronize(st);
        stats_[1] = 1;
        if (e != hipSuccess) return (int)e;
        for (int i = 0; i < B * L; ++i) probs_[i].K = h_counts_[i];
        if (h_counts) memcpy(h_counts, h_counts_, sizeof(int) * B * L);
        prepared_ = true;
        return 0;
    }

    int PairBatch::set_motion(const double *h_cap, const double *h_exp, const double *h_t0, double dt, const double *h_kt, const double *h_kR)
    {
        if (!arena_ || !h_cap || !h_exp || !h_t0 || !h_kt || !h_kR || !(dt > 0)) return MBAVO_E_ARG;
        const int B = plan_.B, L = plan_.L, N = plan_.N, k = opts_.spline_deg_k;
        // every blur sample of every level on knots that exist: the kernels' own sample times (compute_virtual_camera_poses.cu:33),
        // checked on the host as the host-driven tracker does; nothing is touched before every pair has passed
        for (int b = 0; b < B; ++b)
            for (int l = 0; l < L; ++l)
                for (int smp = 0; smp < opts_.S[l]; ++smp)
                {
                    const double ts = h_cap[b] - h_exp[b] * 0.5 + smp * h_exp[b] / (opts_.S[l] - 1 + 1e-8);
                    int idx;
                    double u;
                    spline_segment(ts, h_t0[b], dt, idx, u);
                    if (!(ts == ts) || idx < 0 || idx + k > N) return MBAVO_E_RANGE;
                }
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        double *m = h_motion_;
        memcpy(m, h_cap, sizeof(double) * B);
        memcpy(m + B, h_exp, sizeof(double) * B);
        memcpy(m + 2 * B, h_kt, sizeof(double) * B * 3 * N);
        memcpy(m + 2 * B + (size_t)B * 3 * N, h_kR, sizeof(double) * B * 4 * N);
        hipStream_t st = eng_.stream();
        double *m_t0 = m + (size_t)B * (2 + 7 * N); // (the start times also go to the device: mbavo_pairs_assess samples the spline there)
        memcpy(m_t0, h_t0, sizeof(double) * B);
        if ((e = hipMemcpyAsync(arena_ + plan_.off_motion, m, sizeof(double) * B * (2 + 7 * N), hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        if ((e = hipMemcpyAsync(arena_ + off_t0_, m_t0, sizeof(double) * B, hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return (int)e; // (the staging buffer is free again)
        motion_set_ = true;
        for (int b = 0; b < B; ++b)
        {
            int idx;
            double u;
            spline_segment(h_cap[b], h_t0[b], dt, idx, u); // mbavo_segment_start_index
            start_idx_[b] = idx;
            for (int l = 0; l < L; ++l)
            {
                probs_[(size_t)b * L + l].t0 = h_t0[b];
                probs_[(size_t)b * L + l].dt = dt;
            }
        }
        return 0;
    }

    int PairBatch::get_knots(double *h_kt, double *h_kR)
    {
        if (!arena_ || !h_kt || !h_kR) return MBAVO_E_ARG;
        const int B = plan_.B, N = plan_.N;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        const size_t first = 2 * (size_t)B, n = (size_t)B * 7 * N;
        if ((e = hipMemcpyAsync(h_motion_ + first, arena_ + plan_.off_motion + first * sizeof(double), n * sizeof(double), hipMemcpyDeviceToHost, st)) != hipSuccess)
            return (int)e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return (int)e;
        memcpy(h_kt, h_motion_ + first, sizeof(double) * B * 3 * N);
        memcpy(h_kR, h_motion_ + first + (size_t)B * 3 * N, sizeof(double) * B * 4 * N);
        return 0;
    }

    int PairBatch::update(const unsigned char *d_blur, int n_key, const int *h_key_pairs, const unsigned char *d_sharp, const void *d_depth, int *h_counts)
    {
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L;
        if (!arena_ || !prepared_ || n_key < 0 || n_key > B) return MBAVO_E_ARG;
        if (n_key > 0 && (!h_key_pairs || !d_sharp || !d_depth)) return MBAVO_E_ARG;
        for (int i = 0; i < n_key; ++i)
            if (h_key_pairs[i] < 0 || h_key_pairs[i] >= B || (i > 0 && h_key_pairs[i] <= h_key_pairs[i - 1])) return MBAVO_E_ARG;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        const PairLevelDesc *desc = (const PairLevelDesc *)(arena_ + p.off_desc);
        int *d_counts = (int *)(arena_ + p.off_counts);
        const int *d_keys = (const int *)(step_ + step_off_keys(B));
        upd_stats_[0] = upd_stats_[1] = upd_stats_[2] = 0;
        const int n_cur = d_blur ? B : 0;
        if (n_key + n_cur == 0)
        { // nothing changes
            if (h_counts) for (int i = 0; i < B * L; ++i) h_counts[i] = probs_[i].K;
            return 0;
        }
        const int npx0 = p.H[0] * p.W[0];
        if (n_key > 0)
        {
            memcpy(h_keys_, h_key_pairs, sizeof(int) * n_key);
            if ((e = hipMemcpyAsync((void *)d_keys, h_keys_, sizeof(int) * n_key, hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
            hipLaunchKernelGGL(k_pairs_scatter_level0, dim3((npx0 + 4095) / 4096, n_key), dim3(256), 0, st, desc, L, d_keys, d_sharp, npx0);
            ++upd_stats_[0];
        }
        if (d_blur)
        {
            unsigned char *img = (unsigned char *)arena_ + p.off_img;
            if ((e = hipMemcpy2DAsync(img + (size_t)B * p.img_stride, (size_t)p.img_stride, d_blur, (size_t)npx0, (size_t)npx0, B, hipMemcpyDeviceToDevice, st)) != hipSuccess)
                return (int)e;
        }
        for (int l = 0; l + 1 < L; l += 3)
        { // the pyramids below the images that changed
            const int n = L - 1 - l < 3 ? L - 1 - l : 3;
            hipLaunchKernelGGL(k_pairs_pyr_down_listed, dim3((p.W[l] / 2 + 15) / 16, (p.H[l] / 2 + 15) / 16, n_key + n_cur), dim3(256), 0, st, desc, d_keys,
                               n_key, L, l, n);
            ++upd_stats_[0];
        }
        if (n_key > 0)
        {
            const PairsGrid g = pairs_grid(p);
            const dim3 ggrid(g.blk0[L], n_key);
            if (p.format == 0) hipLaunchKernelGGL(k_pairs_gradients_listed<0>, ggrid, dim3(256), 0, st, desc, g, d_keys);
            else if (p.format == 1) hipLaunchKernelGGL(k_pairs_gradients_listed<1>, ggrid, dim3(256), 0, st, desc, g, d_keys);
            else hipLaunchKernelGGL(k_pairs_gradients_listed<2>, ggrid, dim3(256), 0, st, desc, g, d_keys);
            // (row y of d_depth is the map of pair key_pairs[y])
            upd_stats_[0] += 1 + launch_keypoints(opts_.depth_format, p, g, st, desc, d_counts, opts_.score_threshold, d_depth, depth_conv(), n_key, d_keys);
        }
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        if (n_key > 0)
        {
            if ((e = hipMemcpyAsync(h_counts_, d_counts, sizeof(int) * B * L, hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
            upd_stats_[2] = (long long)sizeof(int) * B * L;
        }
        e = hipStreamSynchronize(st); // (the caller's images are free again)
        upd_stats_[1] = 1;
        if (e != hipSuccess) return (int)e;
        if (n_key > 0)
            for (int i = 0; i < B * L; ++i) probs_[i].K = h_counts_[i]; // (the pairs not listed: their counts as they were)
        if (h_counts) for (int i = 0; i < B * L; ++i) h_counts[i] = probs_[i].K;
        return 0;
    }

    void PairBatch::fill_assess_args(AssessArgs &a, double flow_mag0, double flow_mag1, double max_blur_kernel_mag) const
    {
        const PairsPlan &p = plan_;
        const int B = p.B, N = p.N;
        a.desc = (const PairLevelDesc *)(arena_ + p.off_desc);
        a.counts = (const int *)(arena_ + p.off_counts);
        const double *motion = (const double *)(arena_ + p.off_motion);
        a.cap = motion; a.exp = motion + B; a.kt = motion + 2 * B; a.kR = a.kt + (size_t)B * 3 * N;
        a.t0 = (const double *)(arena_ + off_t0_);
        a.dt = probs_[0].dt;
        for (int i = 0; i < 4; ++i) a.K[i] = opts_.intrinsics[i];
        a.flow_mag0 = flow_mag0; a.flow_mag1 = flow_mag1; a.max_blur_kernel_mag = max_blur_kernel_mag;
        a.L = p.L; a.N = N;
        a.out = (mbavo_pairs_assessment *)step_;
    }

    void PairBatch::fill_track_args(TrackArgs &t) const
    {
        const int B = plan_.B, N = plan_.N;
        double *motion = (double *)(arena_ + plan_.off_motion);
        t.state = (double *)(arena_ + off_state_);
        t.cap = motion; t.exp = motion + B; t.kt = motion + 2 * B; t.kR = t.kt + (size_t)B * 3 * N;
        t.t0 = (double *)(arena_ + off_t0_);
        t.times = (const double *)(arena_ + off_times_);
        t.frames = (mbavo_pairs_frame *)(arena_ + off_frames_);
        t.B = B; t.N = N;
    }

    // [knots_t | knots_R | pad | t0 | state]: what set_states uploads and get_states reads back, in one copy
    int PairBatch::set_states(const mbavo_vo_state *h)
    {
        if (!arena_ || !h) return MBAVO_E_ARG;
        const int B = plan_.B, L = plan_.L, N = plan_.N;
        for (int b = 0; b < B; ++b)
            if (h[b].N != N || h[b].is_first != 0 || !(h[b].dt > 0) || h[b].dt != h[0].dt) return MBAVO_E_ARG;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        const long long first = plan_.off_motion + (long long)sizeof(double) * 2 * B;
        double *kt = (double *)h_state_, *kR = kt + (size_t)B * 3 * N;
        double *t0 = (double *)(h_state_ + (off_t0_ - first)), *sv = (double *)(h_state_ + (off_state_ - first));
        for (int b = 0; b < B; ++b)
        {
            memcpy(kt + (size_t)b * 3 * N, h[b].knots_t, sizeof(double) * 3 * N);
            memcpy(kR + (size_t)b * 4 * N, h[b].knots_R, sizeof(double) * 4 * N);
            t0[b] = h[b].t0;
            double *v = sv + (size_t)b * kStateLen;
            memcpy(v + kStateKeyframe, h[b].T_keyframe, sizeof(double) * 7);
            memcpy(v + kStatePrev, h[b].T_prev_b2w, sizeof(double) * 7);
            memcpy(v + kStateVelocity, h[b].velocity, sizeof(double) * 6);
            v[kStatePrevTime] = h[b].prev_timestamp;
            v[kStateDtFrame] = 0.0;
        }
        hipStream_t st = eng_.stream();
        if ((e = hipMemcpyAsync(arena_ + first, h_state_, (size_t)(off_times_ - first), hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return (int)e; // (the staging buffer is free again)
        state_dt_ = h[0].dt;
        for (int i = 0; i < B * L; ++i) probs_[i].dt = state_dt_;
        for (int b = 0; b < B; ++b)
            for (int l = 0; l < L; ++l) probs_[(size_t)b * L + l].t0 = h[b].t0;
        states_set_ = true;
        pending_ = false;
        return 0;
    }

    int PairBatch::get_states(mbavo_vo_state *h)
    {
        if (!arena_ || !h || !states_set_) return MBAVO_E_ARG;
        const int B = plan_.B, N = plan_.N;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        const long long first = plan_.off_motion + (long long)sizeof(double) * 2 * B;
        hipStream_t st = eng_.stream();
        if ((e = hipMemcpyAsync(h_state_, arena_ + first, (size_t)(off_times_ - first), hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return (int)e;
        const double *kt = (const double *)h_state_, *kR = kt + (size_t)B * 3 * N;
        const double *t0 = (const double *)(h_state_ + (off_t0_ - first)), *sv = (const double *)(h_state_ + (off_state_ - first));
        for (int b = 0; b < B; ++b)
        {
            memset(&h[b], 0, sizeof(h[b]));
            h[b].t0 = t0[b]; h[b].dt = state_dt_; h[b].N = N; h[b].is_first = 0;
            memcpy(h[b].knots_t, kt + (size_t)b * 3 * N, sizeof(double) * 3 * N);
            memcpy(h[b].knots_R, kR + (size_t)b * 4 * N, sizeof(double) * 4 * N);
            const double *v = sv + (size_t)b * kStateLen;
            memcpy(h[b].T_keyframe, v + kStateKeyframe, sizeof(double) * 7);
            memcpy(h[b].T_prev_b2w, v + kStatePrev, sizeof(double) * 7);
            memcpy(h[b].velocity, v + kStateVelocity, sizeof(double) * 6);
            h[b].prev_timestamp = v[kStatePrevTime];
        }
        return 0;
    }

    int PairBatch::predict(const double *h_cap, const double *h_exp)
    {
        if (!arena_ || !prepared_ || !states_set_ || pending_ || !h_cap || !h_exp) return MBAVO_E_ARG;
        const int B = plan_.B, L = plan_.L, N = plan_.N, k = opts_.spline_deg_k;
        const double dt = state_dt_;
        // the host does the time arithmetic only, as set_motion does: nothing is touched before every pair has passed
        for (int b = 0; b < B; ++b)
        {
            const double t0 = h_cap[b] - 0.5 * h_exp[b]; // :131 setStartTime
            for (int l = 0; l < L; ++l)
                for (int smp = 0; smp < opts_.S[l]; ++smp)
                {
                    const double ts = h_cap[b] - h_exp[b] * 0.5 + smp * h_exp[b] / (opts_.S[l] - 1 + 1e-8);
                    int idx;
                    double u;
                    spline_segment(ts, t0, dt, idx, u);
                    if (!(ts == ts) || idx < 0 || idx + k > N) return MBAVO_E_RANGE;
                }
        }
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        pre_stats_[0] = pre_stats_[1] = pre_stats_[2] = 0;
        // (h_times_ is free: the last predict's copy was followed by a commit or a set_states, which synchronise)
        for (int b = 0; b < B; ++b)
        {
            h_times_[b] = h_cap[b]; h_times_[B + b] = h_exp[b]; h_times_[2 * B + b] = h_cap[b] - 0.5 * h_exp[b];
        }
        if ((e = hipMemcpyAsync(arena_ + off_times_, h_times_, sizeof(double) * 3 * B, hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        TrackArgs t;
        fill_track_args(t);
        hipLaunchKernelGGL(k_pairs_predict, dim3((B + 15) / 16), dim3(256), 0, st, t);
        pre_stats_[0] = 1;
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        for (int b = 0; b < B; ++b)
        {
            int idx;
            double u;
            spline_segment(h_cap[b], h_times_[2 * B + b], dt, idx, u); // mbavo_segment_start_index
            start_idx_[b] = idx;
            for (int l = 0; l < L; ++l)
            {
                probs_[(size_t)b * L + l].t0 = h_times_[2 * B + b];
                probs_[(size_t)b * L + l].dt = dt;
            }
        }
        motion_set_ = true; // (times and knots are all there for mbavo_pairs_assess too)
        pending_ = true;
        return 0;
    }

    int PairBatch::commit(double flow_mag0, double flow_mag1, double max_blur_kernel_mag, mbavo_pairs_frame *h_out)
    {
        if (!arena_ || !pending_ || !h_out) return MBAVO_E_ARG;
        const int B = plan_.B;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        com_stats_[0] = com_stats_[1] = com_stats_[2] = 0;
        AssessArgs a;
        fill_assess_args(a, flow_mag0, flow_mag1, max_blur_kernel_mag);
        a.out = nullptr; // (the assessment goes into the frame record)
        TrackArgs t;
        fill_track_args(t);
        if (opts_.spline_deg_k == 2) hipLaunchKernelGGL(k_pairs_commit<2>, dim3(B), dim3(256), 0, st, a, t);
        else hipLaunchKernelGGL(k_pairs_commit<4>, dim3(B), dim3(256), 0, st, a, t);
        com_stats_[0] = 1;
        pending_ = false; // (the state has moved on, whatever the copy below says)
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        if ((e = hipMemcpyAsync(h_frames_, t.frames, sizeof(mbavo_pairs_frame) * B, hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
        com_stats_[2] = (long long)sizeof(mbavo_pairs_frame) * B;
        e = hipStreamSynchronize(st);
        com_stats_[1] = 1;
        if (e != hipSuccess) return (int)e;
        memcpy(h_out, h_frames_, sizeof(mbavo_pairs_frame) * B);
        return 0;
    }

    int PairBatch::assess(double flow_mag0, double flow_mag1, double max_blur_kernel_mag, mbavo_pairs_assessment *h_out)
    {
        if (!arena_ || !prepared_ || !motion_set_ || !h_out) return MBAVO_E_ARG;
        const int B = plan_.B;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        ass_stats_[0] = ass_stats_[1] = ass_stats_[2] = 0;
        AssessArgs a;
        fill_assess_args(a, flow_mag0, flow_mag1, max_blur_kernel_mag);
        if (opts_.spline_deg_k == 2) hipLaunchKernelGGL(k_pairs_assess<2>, dim3(B), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_pairs_assess<4>, dim3(B), dim3(256), 0, st, a);
        ass_stats_[0] = 1;
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        if ((e = hipMemcpyAsync(h_assess_, a.out, sizeof(mbavo_pairs_assessment) * B, hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
        ass_stats_[2] = (long long)sizeof(mbavo_pairs_assessment) * B;
        e = hipStreamSynchronize(st);
        ass_stats_[1] = 1;
        if (e != hipSuccess) return (int)e;
        memcpy(h_out, h_assess_, sizeof(mbavo_pairs_assessment) * B);
        return 0;
    }

    void PairBatch::last_stats(long long out[4]) const
    {
        out[0] = stats_[0]; out[1] = stats_[1]; out[2] = stats_[2];
        out[3] = arena_ ? plan_.total : 0;
    }
} // namespace mbavo

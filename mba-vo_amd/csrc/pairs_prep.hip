// pairs_prep.hip -- the input side of a batch of keyframe pairs (include/mbavo.h: mbavo_pairs_create, _prepare, _update,
// _set_motion, _get_knots, _plan).  The tracker that carries the pairs from frame to frame is pairs_track.hip.
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
//   raw cameras      Undistort.cpp:17-52                      (mbavo_pairs_opts.undistort) the level-0 copies become ONE remap launch through
//                                                             the object's undistortion map (camera_math.h); with undistort = 2 the
//                                                             depth look-ups go through the map too
//   clearance mask                                            (mbavo_pairs_opts.valid_radius, .mask) a pick or a candidate is kept only where
//                                                             the clearance pyramid of the pair's camera has a 1 (keyframe_ops.hip makes
//                                                             it from the map and the caller's stored mask at the camera call and at
//                                                             mbavo_pairs_set_masks); one byte load, no launch more
//   compaction                                                one workgroup per (pair, level): kept picks in row-major cell order
//   corner score     FeatureDetectorSparse.cpp                (mbavo_pairs_set_detector, score = 1) the selection reads the minimum-
//                    (ENUM_SPARSE_SHI_TOMASI)                 eigenvalue score of the windowed structure tensor in place of the gradient
//                                                             magnitude: ONE launch more over all levels (pairs_score.hip), a policy
//                                                             of the selection kernels
//   every candidate  FeatureDetectorSemiDense.cpp:27-43       (mbavo_pairs_opts.every_candidate, in place of the two above) no grid:
//                    without gridSelection                    count, scan, write over 256-pixel segments, one launch more
//   caller's points  blur_aware_direct_tracker.h:17-19        (mbavo_pairs_prepare_points, _update_points, in place of the three above) no
//                                                             detector, no depth map: level-0 points with depths, taken to every level,
//                                                             tested against border and clearance and compacted in ONE launch
//   ... in the raw geometry  CameraUnified.cpp:68-103,        (mbavo_pairs_set_points_geometry(1)) the points are raw pixels of the pair's camera:
//                    DistortionRadTan.cpp:57-80               inverted inside that launch (camera_math.h), a policy of the same kernel
//
// The pyramid tile, the pixel's differences and their formats, the detector's per-pixel functions, the wave's scan of a cell and
// the workgroup prefix sums are called from keyframe_math.h, where the per-image kernels call them too; the grid of a level comes
// from cell_grid (keyframe_ops.hip).  What is written here is the indexing: the (pair, level) parameters live in a device-resident
// table written once at creation, and a workgroup finds its entry from the grid index.  Results are bit-identical to the
// per-image entry points (tests/test_gpu_pairs_prep.py holds every array to them).  All streaming work, HBM-bound.
//
// One kernel per step, for a prepare (every pair) and for an update (the pairs of a device list): a grid row is a pair, found by
// pair_of_row from the nullable list; a prepare is an update of every image without a list.  Each step appears once: device body,
// kernel, launch (PairBatch::refresh, level 0 included).  Whose camera a pair looks through (one for all, or with
// mbavo_pairs_opts.num_cameras the pair's own) is a policy type of the kernels that need to know: MAPS of the remap, CAM of the
// keypoint kernels.
#include "pairs_prep.h"
#include "keyframe_math.h"
#include "pairs_desc.h"
#include "pixel_math.h"
#include "se3_math.h"
#include "vo_frontend.h"
#include <cmath>
#include <cstring>
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <type_traits>

namespace mbavo
{
    namespace pairs
    {
        // largest level-0 image: one row of the strided level-0 copy is a whole image (tested at this size)
        constexpr long long kMaxPixels = 1ll << 22;

        // ---- pyramids: pyr_down_tile over the images that changed; image z < n_key is the keyframe of row z's pair, else pair
        // (z - n_key)'s current frame (a prepare: n_key = B, no list, 2B images); levels l0 + 1 .. l0 + n below level l0 = d[0]
        // (d[2], d[3]: entries of this pair only where n reaches them)
        __device__ __forceinline__ void pyr_down_image(const PairLevelDesc *d, const bool key, const int n)
        {
            pyr_down_tile(key ? d[0].ref : d[0].cur, d[0].H, d[0].W, key ? d[1].ref : d[1].cur, n < 2 ? nullptr : key ? d[2].ref : d[2].cur,
                          n < 3 ? nullptr : key ? d[3].ref : d[3].cur, n);
        }
        __global__ __launch_bounds__(256) void k_pairs_pyr_down(const PairLevelDesc *__restrict__ desc, const int *__restrict__ key_pairs, int n_key,
                                                                int L, int l0, int n)
        {
            const int z = blockIdx.z;
            pyr_down_image(desc + (size_t)(z < n_key ? pair_of_row(key_pairs, z) : z - n_key) * L + l0, z < n_key, n);
        }

        // ---- gradients of all levels of the rows' keyframes.  A level is walked as a flat array of H*W pixels so that every lane
        // stores 16 aligned bytes whatever the row length (odd widths included): 2 pixels of float pairs, 4 pixels of half pairs or
        // packed words.  The level's slice is padded to 16 pixels, so the last lane's store stays inside it (zeros in the pad).
        template <int FORMAT>
        __device__ __forceinline__ void gradients_of_pair(const PairLevelDesc *__restrict__ desc, const PairsGrid &g, const int pair)
        {
            typedef typename GradPixel<FORMAT>::type Px;
            constexpr int PPL = 16 / (int)sizeof(Px);
            int l = 0;
            while (l + 1 < g.L && (int)blockIdx.x >= g.blk0[l + 1]) ++l;
            const PairLevelDesc &d = desc[(size_t)pair * g.L + l];
            const int H = d.H, W = d.W, npx = H * W;
            const int i0 = (((int)blockIdx.x - g.blk0[l]) * 256 + (int)threadIdx.x) * PPL;
            if (i0 >= npx) return;
            const unsigned char *__restrict__ src = d.ref;
            int y = i0 / W, x = i0 - y * W;
            alignas(16) Px out[PPL];
#pragma unroll
            for (int j = 0; j < PPL; ++j)
            {
                const int i = i0 + j;
                int I = 0, kx = 0, ky = 0;
                if (i < npx)
                {
                    I = (int)src[i];
                    central_diff(src, H, W, x, y, i, kx, ky);
                }
                out[j] = GradPixel<FORMAT>::of(I, kx, ky);
                if (++x == W) { x = 0; ++y; }
            }
            uint4 v;
            __builtin_memcpy(&v, out, 16);
            *reinterpret_cast<uint4 *>((char *)d.grad + (size_t)i0 * sizeof(Px)) = v;
        }
        template <int FORMAT>
        __global__ __launch_bounds__(256) void k_pairs_gradients(const PairLevelDesc *__restrict__ desc, const PairsGrid g,
                                                                 const int *__restrict__ key_pairs)
        {
            gradients_of_pair<FORMAT>(desc, g, pair_of_row(key_pairs, (int)blockIdx.y));
        }

        // ---- CAM, the last argument of the kernels that look depths up (k_pairs_detect, k_pairs_dense_count, _dense_write): the
        // camera of a grid row's pair -- its DepthConv and its raw-depth look-up (RAW: NoRawDepth, or with
        // mbavo_pairs_opts.undistort = 2 the RawDepth whose Hs x Ws maps are looked up through the undistortion map:
        // keyframe_math.h).
        // CLR is the clearance test of mbavo_pairs_opts.valid_radius (include/mbavo.h): NoClearance, an empty kernel argument that
        // keeps every pixel, or with valid_radius > 0 the Clearance of the pair's camera -- the base of its pyramid of bytes; the
        // level's first byte is PairLevelDesc::clear0.  One byte load per pick or per candidate.
        // OneCamera: the object's one camera, by value and whatever the pair (the conversion's constants come last: a float z map
        // does not read them).
        // GEO, the geometry a caller's points come in (k_pairs_points; mbavo_pairs_set_points_geometry): SameGeometry, the
        // object's undistorted geometry -- no code; RawGeometry, the raw camera's -- a point outside the Hs x Ws raw image has no
        // pixel (NaN: unusable at every level), the others go through the inverse camera (camera_math.h: undistorted_position).
        struct SameGeometry
        {
            __device__ __forceinline__ void to_undistorted(double &, double &) const {}
        };
        struct RawGeometry
        {
            const MapCamera *cam;
            int Hs, Ws;
            __device__ __forceinline__ void to_undistorted(double &x, double &y) const
            {
                const double u = x, v = y;
                if (!raw_point_inside(u, v, Hs, Ws)) { x = y = __builtin_nan(""); return; }
                undistorted_position(*cam, u, v, x, y);
            }
        };
        // RSP, the response the selection reads (mbavo_pairs_set_detector): a camera policy names it as it names the clearance.
        // ByGradient, an empty value: the gradient magnitude of the level's bytes, the object as created.  ByScore: the float at the
        // pixel's index of the (pair, level)'s score slice, which k_pairs_score (pairs_score.hip) has filled before the selection.
        struct ByGradient
        {
            __device__ __forceinline__ GradientResponse at_level(const PairLevelDesc &) const { return GradientResponse{}; }
        };
        struct ByScore
        {
            ScoreSlices slices;
            __device__ __forceinline__ ScoreResponse at_level(const PairLevelDesc &d) const { return ScoreResponse{slices.of(d)}; }
        };
        struct NoClearance
        {
            __device__ __forceinline__ bool clear(int, int) const { return true; }
        };
        struct Clearance
        {
            const unsigned char *bytes;
            __device__ __forceinline__ bool clear(int level0, int i) const { return bytes[(size_t)level0 + (size_t)i] != 0; }
        };
        template <class RAW, class CLR = NoClearance>
        struct OneCamera
        {
            DepthConv dc;
            [[no_unique_address]] RAW raw;
            [[no_unique_address]] CLR clr;
            __device__ __forceinline__ const DepthConv &depth_conv(int) const { return dc; }
            __device__ __forceinline__ const RAW &raw_depth(int) const { return raw; }
            __device__ __forceinline__ const CLR &clearance(int) const { return clr; }
            __device__ __forceinline__ SameGeometry points_geometry(int) const { return SameGeometry{}; }
            __device__ __forceinline__ ByGradient response(int) const { return ByGradient{}; }
            static constexpr bool kCameraSet = false;
        };
        // PairCameras (mbavo_pairs_opts.num_cameras > 0): the four intrinsics of DepthConv and, RAW_DEPTH (undistort = 2), the map
        // RawDepth looks through come from the pair's entry of the camera arrays -- one entry per grid row, scalar loads.
        // CLEAR (valid_radius > 0): the pyramid of the pair's camera, ClearSet::base + cam * stride.
        template <bool RAW_DEPTH, bool CLEAR = false>
        struct PairCameras
        {
            CameraSet cs;
            struct NoClearSet
            {
            };
            [[no_unique_address]] std::conditional_t<CLEAR, ClearSet, NoClearSet> cl;
            __device__ __forceinline__ auto clearance(int pair) const
            {
                if constexpr (CLEAR) return Clearance{cl.base + (size_t)cs.of_pair[pair].cam * (size_t)cl.stride};
                else return NoClearance{};
            }
            __device__ __forceinline__ DepthConv depth_conv(int pair) const
            {
                const PairCamera &pc = cs.of_pair[pair];
                DepthConv c;
                c.fx = pc.fx; c.fy = pc.fy; c.cx = pc.cx; c.cy = pc.cy;
                c.unit = cs.unit; c.max = cs.max;
                return c;
            }
            __device__ __forceinline__ auto raw_depth(int pair) const
            {
                if constexpr (RAW_DEPTH) return RawDepth{cs.maps + (size_t)cs.of_pair[pair].cam * (size_t)cs.map_floats, cs.Hs, cs.Ws};
                else return NoRawDepth{};
            }
            __device__ __forceinline__ SameGeometry points_geometry(int) const { return SameGeometry{}; }
            __device__ __forceinline__ ByGradient response(int) const { return ByGradient{}; }
            static constexpr bool kCameraSet = true;
        };
        // ScoredCamera (mbavo_pairs_set_detector, score = 1): a camera policy CAM of the detector kernels whose response is the corner
        // score -- depth, raw depth and clearance are CAM's.
        template <class CAM>
        struct ScoredCamera
        {
            CAM cam;
            ScoreSlices slices;
            __device__ __forceinline__ decltype(auto) depth_conv(int pair) const { return cam.depth_conv(pair); }
            __device__ __forceinline__ decltype(auto) raw_depth(int pair) const { return cam.raw_depth(pair); }
            __device__ __forceinline__ decltype(auto) clearance(int pair) const { return cam.clearance(pair); }
            __device__ __forceinline__ ByScore response(int) const { return ByScore{slices}; }
        };
        // RawPoints (mbavo_pairs_set_points_geometry(1)): a camera policy CAM of the points kernel whose points come in the raw
        // geometry -- the clearance is CAM's, the geometry that of the pair's raw camera: the object's one camera by value
        // (OneRawCamera) or the pair's entry of the set's device array (SetRawCameras; a scalar load per grid row).
        struct OneRawCamera
        {
            MapCamera cam;
            int Hs, Ws;
            __device__ __forceinline__ RawGeometry of_pair(int) const { return RawGeometry{&cam, Hs, Ws}; }
        };
        struct SetRawCameras
        {
            const MapCamera *cams;      // G
            const PairCamera *pair_cam; // B
            int Hs, Ws;
            __device__ __forceinline__ RawGeometry of_pair(int pair) const { return RawGeometry{cams + pair_cam[pair].cam, Hs, Ws}; }
        };
        template <class CAM, class RAWCAM>
        struct RawPoints
        {
            CAM cam;
            RAWCAM raw;
            __device__ __forceinline__ auto clearance(int pair) const { return cam.clearance(pair); }
            __device__ __forceinline__ RawGeometry points_geometry(int pair) const { return raw.of_pair(pair); }
        };

        // ---- grid selection: best_pixel_in_cell as detect_cell of keyframe_ops.hip calls it, then the pair's depth map and the border
        // test; one wave per cell, four cells per workgroup; grid (ceil(cells of a pair / 4), rows)
        // (`pair`: whose levels; the depth map is row blockIdx.y of depth_all -- the same thing in a prepare, the pair's place in the
        // list in an update -- in the element size of the depth format DF: keyframe_math.h)
        template <int DF, class RAW>
        __device__ __forceinline__ const typename DepthMap<DF>::elem *depth_row(const void *__restrict__ depth_all, int H0, int W0, const RAW &raw)
        {
            return static_cast<const typename DepthMap<DF>::elem *>(depth_all) + (size_t)blockIdx.y * depth_map_elems(raw, H0, W0);
        }
        template <int DF, class RAW, class CLR, class RSP>
        __device__ __forceinline__ void detect_cell_of_pair(const PairLevelDesc *__restrict__ desc, const PairsGrid &g, const int pair, float thr,
                                                            const void *__restrict__ depth_all, int H0, int W0, const DepthConv &dc, const RAW &raw,
                                                            const CLR &clr, const RSP &rsp)
        {
            const int lane = threadIdx.x & 63, cell = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
            if (cell >= g.cell0[g.L]) return; // (whole waves)
            int l = 0;
            while (l + 1 < g.L && cell >= g.cell0[l + 1]) ++l;
            const PairLevelDesc &d = desc[(size_t)pair * g.L + l];
            const unsigned char *__restrict__ src = d.ref;
            const int H = d.H, W = d.W, cell_h = d.ch, cell_w = d.cw, ci = cell - g.cell0[l];
            float best;
            int best_idx;
            best_pixel_in_cell(rsp.at_level(d), src, H, W, (ci / d.cells_w) * cell_h, (ci % d.cells_w) * cell_w, cell_h, cell_w, thr, lane, best, best_idx);
            if (lane == 0)
            {
                CellPick p = pick_at(best, best_idx, W);
                if (p.keep)
                {
                    const typename DepthMap<DF>::elem *depth = depth_row<DF>(depth_all, H0, W0, raw); // the pair's own map
                    const int m = d.border;
                    const bool inside = p.x >= m && p.x < W - m && p.y >= m && p.y < H - m;
                    p.keep = (depth_of<DF>(depth, W0, d.scale, p.x, p.y, dc, raw, p.z) && inside) ? 1 : 0;
                    if (p.keep && !clr.clear(d.clear0, best_idx)) p.keep = 0; // (AND with the border test; NoClearance: no code)
                }
                d.picks[ci] = p;
            }
        }
        template <int DF, class CAM>
        __global__ __launch_bounds__(256) void k_pairs_detect(const PairLevelDesc *__restrict__ desc, const PairsGrid g, float thr,
                                                              const void *__restrict__ depth_all, int H0, int W0,
                                                              const int *__restrict__ key_pairs, const CAM cam)
        {
            const int pair = pair_of_row(key_pairs, (int)blockIdx.y);
            detect_cell_of_pair<DF>(desc, g, pair, thr, depth_all, H0, W0, cam.depth_conv(pair), cam.raw_depth(pair), cam.clearance(pair),
                                    cam.response(pair));
        }

        // ---- ordered compaction: one workgroup per (pair, level), grid (L, rows).  256 cells per step: a kept pick's place is
        // (kept so far) + (kept picks of earlier lanes: block_rank_of_flag).
        __device__ __forceinline__ void compact_entry(const PairLevelDesc *__restrict__ desc, int *__restrict__ counts, const int e)
        {
            __shared__ int wave_total[4];
            const PairLevelDesc &d = desc[e];
            const int n = d.cells;
            int base = 0;
            for (int c0 = 0; c0 < n; c0 += 256)
            {
                const int i = c0 + (int)threadIdx.x;
                CellPick p;
                p.keep = 0; p.x = 0; p.y = 0; p.z = 0.f;
                if (i < n) p = d.picks[i];
                int total;
                const int pos = base + block_rank_of_flag(p.keep != 0, wave_total, total); // < cells: one pick per cell at most
                if (p.keep)
                {
                    reinterpret_cast<double2 *>(d.kp_xy)[pos] = make_double2((double)p.x, (double)p.y);
                    d.kp_z[pos] = (double)p.z;
                }
                base += total;
                __syncthreads(); // (wave_total is rewritten in the next step)
            }
            if (threadIdx.x == 0) counts[e] = base;
        }
        __global__ __launch_bounds__(256) void k_pairs_compact(const PairLevelDesc *__restrict__ desc, int *__restrict__ counts,
                                                               const int *__restrict__ key_pairs)
        {
            compact_entry(desc, counts, pair_of_row(key_pairs, (int)blockIdx.y) * (int)gridDim.x + (int)blockIdx.x);
        }

        // ---- keypoints from the caller (mbavo_pairs_prepare_points, _update_points: include/mbavo.h): no detector and no depth
        // map -- grid row y brings the level-0 points offsets[y] .. offsets[y + 1] - 1 of (xy, z).  One workgroup per (pair, level),
        // grid (L, rows), 256 points per step: a lane loads its point (16 + 8 bytes, consecutive lanes consecutive points), takes
        // it to the level, tests it where a pick is tested (border, clearance) and stores it at (kept so far) + (kept points of
        // earlier lanes) -- compact_entry's order, so the list's order is kept.  A row is at most the smallest capacity of the
        // levels long (checked on the host), so every place is inside the level's slice.  Raw points (GEO = RawGeometry) become
        // points of the undistorted geometry right after the load; every level's workgroup inverts the camera for itself -- no
        // scratch, no launch more.
        template <class CLR>
        __device__ __forceinline__ bool point_at_level(const PairLevelDesc &d, const double s, const double x0, const double y0, const double z,
                                                       const CLR &clr, int &xi, int &yi)
        {
            const double xl = x0 / s, yl = y0 / s; // (s a power of two: exact)
            if (!(fabs(xl) < 1073741824.0 && fabs(yl) < 1073741824.0)) return false; // (NaN and +-inf fail)
            xi = (int)floor(xl + 0.5); yi = (int)floor(yl + 0.5);
            if (z < 1e-2 || !(fabs(z) <= 1.7976931348623157e308)) return false; // (no depth; NaN and +-inf)
            const int m = d.border;
            if (!(xi >= m && xi < d.W - m && yi >= m && yi < d.H - m)) return false;
            return clr.clear(d.clear0, yi * d.W + xi); // (AND with the border test; NoClearance: no code)
        }
        template <class CLR, class GEO>
        __device__ __forceinline__ void points_entry(const PairLevelDesc *__restrict__ desc, int *__restrict__ counts, const int e, const int level,
                                                     const double *__restrict__ xy, const double *__restrict__ z, const int first, const int last,
                                                     const CLR &clr, const GEO &geo)
        {
            __shared__ int wave_total[4];
            const PairLevelDesc &d = desc[e];
            const double s = (double)(1 << level);
            double2 *__restrict__ kp_xy = reinterpret_cast<double2 *>(d.kp_xy);
            double *__restrict__ kp_z = d.kp_z;
            int base = 0;
            for (int c0 = first; c0 < last; c0 += 256)
            {
                const int i = c0 + (int)threadIdx.x;
                int xi = 0, yi = 0;
                double zi = 0.0;
                bool keep = false;
                if (i < last)
                {
                    double x0 = xy[2 * (size_t)i], y0 = xy[2 * (size_t)i + 1]; // (two loads: the caller's array is 8-byte aligned only)
                    zi = z[i];
                    geo.to_undistorted(x0, y0); // (SameGeometry: no code)
                    keep = point_at_level(d, s, x0, y0, zi, clr, xi, yi);
                }
                int total;
                const int pos = base + block_rank_of_flag(keep, wave_total, total); // < last - first <= the level's capacity
                if (keep)
                {
                    kp_xy[pos] = make_double2((double)xi, (double)yi);
                    kp_z[pos] = zi;
                }
                base += total;
                __syncthreads(); // (wave_total is rewritten in the next step)
            }
            if (threadIdx.x == 0) counts[e] = base;
        }
        template <class CAM>
        __global__ __launch_bounds__(256) void k_pairs_points(const PairLevelDesc *__restrict__ desc, int *__restrict__ counts,
                                                              const int *__restrict__ key_pairs, const int *__restrict__ offsets,
                                                              const double *__restrict__ xy, const double *__restrict__ z, const CAM cam)
        {
            const int pair = pair_of_row(key_pairs, (int)blockIdx.y);
            points_entry(desc, counts, pair * (int)gridDim.x + (int)blockIdx.x, (int)blockIdx.x, xy, z,
                         offsets[blockIdx.y], offsets[blockIdx.y + 1], cam.clearance(pair), cam.points_geometry(pair));
        }

        // ---- every candidate (mbavo_pairs_opts.every_candidate): row_candidate of keyframe_ops.hip with the border test, all
        // levels of the rows' pairs in three launches.  A level is walked as a flat array of H*W pixels in segments of 256: a wave owns one
        // segment (four steps of 64 pixels, so its candidates are contiguous in row-major order), a workgroup four of them; the
        // workgroups of a pair's levels lie side by side in blockIdx.x (PairsGrid::cell0).  Count, scan, write: the order comes
        // from the scan alone -- no workgroup waits on another and nothing is atomic, so the result is deterministic.
        constexpr int kSegPixels = 256, kSegsPerGroup = 4;
        template <int DF, class RAW, class CLR, class RESP>
        __device__ __forceinline__ bool dense_candidate(const PairLevelDesc &d, float thr, const typename DepthMap<DF>::elem *__restrict__ depth, int W0,
                                                        const DepthConv &dc, const RAW &raw, const CLR &clr, const RESP &resp, int i, int &x, int &y,
                                                        float &z)
        {
            if (i >= d.H * d.W) return false;
            y = i / d.W; x = i - y * d.W;
            const int m = d.border;
            if (!(x >= m && x < d.W - m && y >= m && y < d.H - m)) return false;
            if (!clr.clear(d.clear0, i)) return false; // (before the gradient and the depth: a masked pixel is the cheapest)
            const float g = resp.at(d.ref, d.H, d.W, x, y);
            if (!(g > thr)) return false;
            return depth_of<DF>(depth, W0, d.scale, x, y, dc, raw, z); // (x < W_l = W0 >> l: its level-0 position is inside the map)
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
        template <int DF, class RAW, class CLR, class RSP>
        __device__ __forceinline__ void dense_count_of_pair(const PairLevelDesc *__restrict__ desc, const PairsGrid &g, const int pair, float thr,
                                                            const void *__restrict__ depth_all, int H0, int W0, const DepthConv &dc, const RAW &raw,
                                                            const CLR &clr, const RSP &rsp)
        {
            const PairLevelDesc *d;
            int seg;
            if (!dense_segment(desc, g, pair, d, seg)) return;
            const typename DepthMap<DF>::elem *depth = depth_row<DF>(depth_all, H0, W0, raw); // the pair's own map (as detect_cell_of_pair)
            const auto resp = rsp.at_level(*d);
            const int lane = threadIdx.x & 63;
            int n = 0;
#pragma unroll
            for (int s = 0; s < kSegPixels / 64; ++s)
            {
                int x, y;
                float z;
                n += __popcll(__ballot(dense_candidate<DF>(*d, thr, depth, W0, dc, raw, clr, resp, seg * kSegPixels + s * 64 + lane, x, y, z)));
            }
            if (lane == 0) d->seg[seg] = n;
        }
        template <int DF, class CAM>
        __global__ __launch_bounds__(256) void k_pairs_dense_count(const PairLevelDesc *__restrict__ desc, const PairsGrid g, float thr,
                                                                   const void *__restrict__ depth_all, int H0, int W0,
                                                                   const int *__restrict__ key_pairs, const CAM cam)
        {
            const int pair = pair_of_row(key_pairs, (int)blockIdx.y);
            dense_count_of_pair<DF>(desc, g, pair, thr, depth_all, H0, W0, cam.depth_conv(pair), cam.raw_depth(pair), cam.clearance(pair),
                                    cam.response(pair));
        }

        // in-place exclusive scan of an entry's segment counts, one workgroup per (pair, level), grid (L, rows); 256 segments per
        // step (block_exclusive_scan).  The total is the entry's K.
        __device__ __forceinline__ void dense_scan_entry(const PairLevelDesc *__restrict__ desc, int *__restrict__ counts, const int e)
        {
            __shared__ int wave_total[4];
            const PairLevelDesc &d = desc[e];
            const int n = (d.H * d.W + kSegPixels - 1) / kSegPixels;
            int *__restrict__ seg = d.seg;
            int base = 0;
            for (int c0 = 0; c0 < n; c0 += 256)
            {
                const int i = c0 + (int)threadIdx.x;
                int total;
                const int before = block_exclusive_scan(i < n ? seg[i] : 0, wave_total, total);
                if (i < n) seg[i] = base + before;
                base += total;
                __syncthreads(); // (wave_total is rewritten in the next step)
            }
            if (threadIdx.x == 0) counts[e] = base;
        }
        __global__ __launch_bounds__(256) void k_pairs_dense_scan(const PairLevelDesc *__restrict__ desc, int *__restrict__ counts,
                                                                  const int *__restrict__ key_pairs)
        {
            dense_scan_entry(desc, counts, pair_of_row(key_pairs, (int)blockIdx.y) * (int)gridDim.x + (int)blockIdx.x);
        }

        // the predicate again, the same bits; a candidate's place is (candidates before its segment) + (earlier steps of the wave)
        // + (earlier lanes): < K <= H*W, the entry's capacity
        template <int DF, class RAW, class CLR, class RSP>
        __device__ __forceinline__ void dense_write_of_pair(const PairLevelDesc *__restrict__ desc, const PairsGrid &g, const int pair, float thr,
                                                            const void *__restrict__ depth_all, int H0, int W0, const DepthConv &dc, const RAW &raw,
                                                            const CLR &clr, const RSP &rsp)
        {
            const PairLevelDesc *d;
            int seg;
            if (!dense_segment(desc, g, pair, d, seg)) return;
            const typename DepthMap<DF>::elem *depth = depth_row<DF>(depth_all, H0, W0, raw);
            const auto resp = rsp.at_level(*d);
            const int lane = threadIdx.x & 63;
            double2 *__restrict__ kp_xy = reinterpret_cast<double2 *>(d->kp_xy);
            double *__restrict__ kp_z = d->kp_z;
            int pos = d->seg[seg];
#pragma unroll
            for (int s = 0; s < kSegPixels / 64; ++s)
            {
                int x = 0, y = 0;
                float z = 0.f;
                const bool c = dense_candidate<DF>(*d, thr, depth, W0, dc, raw, clr, resp, seg * kSegPixels + s * 64 + lane, x, y, z);
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
        template <int DF, class CAM>
        __global__ __launch_bounds__(256) void k_pairs_dense_write(const PairLevelDesc *__restrict__ desc, const PairsGrid g, float thr,
                                                                   const void *__restrict__ depth_all, int H0, int W0,
                                                                   const int *__restrict__ key_pairs, const CAM cam)
        {
            const int pair = pair_of_row(key_pairs, (int)blockIdx.y);
            dense_write_of_pair<DF>(desc, g, pair, thr, depth_all, H0, W0, cam.depth_conv(pair), cam.raw_depth(pair), cam.clearance(pair),
                                    cam.response(pair));
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

        // ---- (mbavo_pairs_opts.undistort) level 0 of the images that changed, remapped from the raw camera's Hs x Ws images in
        // place of the copies: image y < n_key is the new keyframe of row y's pair, else pair (y - n_key)'s current frame (a
        // prepare: n_key = B, no list, 2B images).  Four destination pixels per lane, one word (the destination is 256-byte
        // aligned, as the map; the taps are byte loads: a raw image starts wherever y * Hs * Ws falls).
        // MAPS: whose map a pair's images go through.  SharedMap: the object's one map (mbavo_pairs_set_camera*).  CameraMaps
        // (mbavo_pairs_opts.num_cameras > 0): the map of the pair's camera, maps + camera_of_pair * 2 H W floats -- the index is the
        // same for the whole grid row (a scalar load), and a map that starts off a 16-byte boundary (H W odd) takes remap_four's
        // byte-wise branch for that row: the same bytes.
        struct SharedMap
        {
            const float *map;
            __device__ __forceinline__ const float *of_pair(int) const { return map; }
        };
        struct CameraMaps
        {
            const float *maps;
            const PairCamera *cams;
            long long map_floats;
            __device__ __forceinline__ const float *of_pair(int pair) const { return maps + (size_t)cams[pair].cam * (size_t)map_floats; }
        };
        template <class MAPS>
        __global__ __launch_bounds__(256) void k_pairs_remap_level0(const PairLevelDesc *__restrict__ desc, int L, const int *__restrict__ key_pairs,
                                                                    int n_key, const unsigned char *__restrict__ raw_key,
                                                                    const unsigned char *__restrict__ raw_cur, int Hs, int Ws,
                                                                    const MAPS maps, int npx)
        {
            const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
            if (i0 >= npx) return;
            const int y = blockIdx.y;
            const bool key = y < n_key;
            const unsigned char *__restrict__ src = (key ? raw_key : raw_cur) + (size_t)(key ? y : y - n_key) * Hs * Ws;
            const int pair = key ? pair_of_row(key_pairs, y) : y - n_key;
            const PairLevelDesc &d = desc[(size_t)pair * L];
            remap_four<1>({src}, Hs, Ws, maps.of_pair(pair), {key ? d.ref : d.cur}, npx, i0);
        }

        // (a prepare of an object with a set of cameras) both images of a pair in one lane: the keyframe and the current frame of
        // pair blockIdx.y go through the same four map entries, read once (camera_math.h: remap_four<2>), where the kernel above
        // reads them in two grid rows.  With one map per pair that halves the map bytes of the launch.  The same bytes out.
        __global__ __launch_bounds__(256) void k_pairs_remap_level0_both(const PairLevelDesc *__restrict__ desc, int L,
                                                                         const unsigned char *__restrict__ raw_key,
                                                                         const unsigned char *__restrict__ raw_cur, int Hs, int Ws,
                                                                         const CameraMaps maps, int npx)
        {
            const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
            if (i0 >= npx) return;
            const int pair = blockIdx.y;
            const float *__restrict__ map = maps.of_pair(pair);
            const PairLevelDesc &d = desc[(size_t)pair * L];
            const size_t off = (size_t)pair * Hs * Ws;
            remap_four<2>({raw_key + off, raw_cur + off}, Hs, Ws, map, {d.ref, d.cur}, npx, i0);
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

    // The keypoint launches over `rows` keyframes (d_keys null: row = pair; else row = the pair's place in the key list), reading
    // the depth maps in format DF through the camera policy `cam`; the number of launches.
    template <int DF, class CAM>
    static int launch_keypoints(const PairsPlan &p, const PairsGrid &g, hipStream_t st, const PairLevelDesc *desc, int *d_counts, float thr,
                                const void *d_depth, int rows, const int *d_keys, const CAM &cam)
    {
        const int L = p.L, H0 = p.H[0], W0 = p.W[0];
        if (p.dense)
        { // every candidate: count, scan, write
            const dim3 grid(g.cell0[L], rows);
            hipLaunchKernelGGL((k_pairs_dense_count<DF, CAM>), grid, dim3(256), 0, st, desc, g, thr, d_depth, H0, W0, d_keys, cam);
            hipLaunchKernelGGL(k_pairs_dense_scan, dim3(L, rows), dim3(256), 0, st, desc, d_counts, d_keys);
            hipLaunchKernelGGL((k_pairs_dense_write<DF, CAM>), grid, dim3(256), 0, st, desc, g, thr, d_depth, H0, W0, d_keys, cam);
            return 3;
        }
        hipLaunchKernelGGL((k_pairs_detect<DF, CAM>), dim3((p.cell0[L] + 3) / 4, rows), dim3(256), 0, st, desc, g, thr, d_depth, H0, W0, d_keys, cam);
        hipLaunchKernelGGL(k_pairs_compact, dim3(L, rows), dim3(256), 0, st, desc, d_counts, d_keys);
        return 2;
    }
    template <class CAM>
    static int launch_keypoints(int depth_format, const PairsPlan &p, const PairsGrid &g, hipStream_t st, const PairLevelDesc *desc, int *d_counts,
                                float thr, const void *d_depth, int rows, const int *d_keys, const CAM &cam)
    {
        if (depth_format == 0) return launch_keypoints<0>(p, g, st, desc, d_counts, thr, d_depth, rows, d_keys, cam);
        if (depth_format == 1) return launch_keypoints<1>(p, g, st, desc, d_counts, thr, d_depth, rows, d_keys, cam);
        return launch_keypoints<2>(p, g, st, desc, d_counts, thr, d_depth, rows, d_keys, cam);
    }

    // The caller's points in place of the detector: ONE launch, whatever the object's keypoint mode and depth format are.
    template <class CAM>
    static int launch_points(const PairsPlan &p, hipStream_t st, const PairLevelDesc *desc, int *d_counts, int rows, const int *d_keys,
                             const KeypointSource &src, const CAM &cam)
    {
        hipLaunchKernelGGL(k_pairs_points<CAM>, dim3(p.L, rows), dim3(256), 0, st, desc, d_counts, d_keys, src.d_offsets, src.d_xy, src.d_z, cam);
        return 1;
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
        if (o->undistort < 0 || o->undistort > 2) return MBAVO_E_ARG;
        if (o->num_cameras < 0 || o->num_cameras > B) return MBAVO_E_ARG;
        if (o->mask != 0 && o->mask != 1) return MBAVO_E_ARG;
        if (o->valid_radius < 0 || o->valid_radius > kClearMaxRadius || (o->valid_radius > 0 && o->undistort == 0 && o->mask == 0)) return MBAVO_E_ARG;
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
                // (level l is (H >> l) x (W >> l) = the size the grid is made for: every pixel's cell exists, so detect_semidense's
                // MBAVO_E_RANGE -- an image larger than the grid of the H0 x W0 it is given -- cannot occur here)
                CellGrid g;
                const int rc = cell_grid(o->H, o->W, l, o->cell_H, o->cell_W, Hl, Wl, g);
                if (rc != 0) return rc;
                p.ch[l] = g.ch; p.cw[l] = g.cw; p.cells_w[l] = g.cells_w; p.cells[l] = g.cells_h * g.cells_w;
                p.cap[l] = p.cells[l];
                p.cell0[l + 1] = p.cell0[l] + p.cells[l];
            }
            p.px0[l + 1] = p.px0[l] + align_up((long long)Hl * Wl, 16);
            p.kp0[l + 1] = p.kp0[l] + 3ll * align_up(p.cap[l], 2);
            p.pat0[l + 1] = p.pat0[l] + 2 * o->P[l];
            p.clear0[l + 1] = p.clear0[l] + align_up((long long)Hl * Wl, kAlign);
        }
        p.clear_stride = p.clear0[L];
        p.mask_stride = align_up((long long)o->H * o->W, kAlign);
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
        // (one level-0 map for all pairs, or one per camera of the set; undistort = 0: nothing, no offset moves)
        p.off_map = take(o->undistort != 0 ? 8ll * o->H * o->W * (o->num_cameras > 0 ? o->num_cameras : 1) : 0);
        // (one clearance pyramid per map; valid_radius = 0 without masks: nothing, no offset moves)
        p.off_clear = take(o->valid_radius > 0 || o->mask ? p.clear_stride * (o->num_cameras > 0 ? o->num_cameras : 1) : 0);
        // (mask = 1: one stored level-0 mask per camera; else nothing, no offset moves)
        p.off_mask = take(o->mask ? p.mask_stride * (o->num_cameras > 0 ? o->num_cameras : 1) : 0);
        p.off_motion = take((long long)B * (2 + 7 * o->N) * 8);
        p.total = at;
        return 0;
    }

    // the tail sits behind the plan's arrays, in the same allocation, so that knots and state move in ONE copy (pairs_prep.h)
    PairsArena::PairsArena(const PairsPlan &p, int G) : plan(p)
    {
        const long long B = p.B, N = p.N, d = sizeof(double);
        o_exp = p.off_motion + d * B; o_knots_t = o_exp + d * B; o_knots_R = o_knots_t + d * B * 3 * N;
        long long at = p.total;
        auto take = [&at](long long n) { const long long o_ = at; at += align_up(n, kAlign); return o_; };
        o_t0 = take(d * B);
        o_state = take(d * kStateLen * B);
        span_first = o_knots_t; span_bytes = at - span_first;
        o_times = take(d * 3 * B);
        o_frames = take((long long)sizeof(mbavo_pairs_frame) * B);
        cams_bytes = G > 0 ? (long long)sizeof(MapCamera) * G + (long long)sizeof(PairCamera) * B : 0;
        o_map_cams = take(cams_bytes);
        o_pair_cams = o_map_cams + (long long)sizeof(MapCamera) * G;
        bytes = at;
    }

    PairBatch::~PairBatch() // (the buffers free themselves and the depth calls destroy their events behind this)
    {
        if (cams_copied_) (void)hipEventDestroy(cams_copied_);
        if (!arena_) return; // (create's first allocation: without it there is no other)
        (void)hipSetDevice(eng_.device());
        (void)hipStreamSynchronize(eng_.stream());
    }

    int PairBatch::create(const mbavo_pairs_opts *o)
    {
        PairsPlan plan;
        int rc = pairs_plan(o, plan);
        if (rc != 0) return rc;
        lay_ = PairsArena(plan, o->num_cameras);
        const PairsArena &a = lay_;
        const PairsPlan &p = a.plan;
        const int B = p.B, L = p.L, N = p.N;
        opts_ = *o;
        slots_ = DepthSlots(p);
        // (the A/B switch of tools/pairs_cameras_bench.py: MBAVO_PAIRS_REMAP_BOTH=0 remaps a prepare's images in 2B grid rows)
        remap_both_ = opt_flag(0, read_env_overrides().pairs_remap_both, true);
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        // (the row pass of the clearance kernels writes into the context's scratch: reserved here, so that a camera call never grows it)
        if (o->valid_radius > 0 && !eng_.named_scratch(kClearWorkSlot, (size_t)p.clear_stride * (size_t)cameras()))
            return (int)hipErrorOutOfMemory;
        // (the offsets of a points call travel through the context's scratch too: B + 1 ints, reserved here)
        if (!eng_.named_scratch(kPointOffsetsSlot, sizeof(int) * ((size_t)B + 1))) return (int)hipErrorOutOfMemory;
        if (o->num_cameras > 0 && (e = hipEventCreateWithFlags(&cams_copied_, hipEventDisableTiming)) != hipSuccess) { cams_copied_ = nullptr; return (int)e; }
        // the object's buffers, in this order; one that cannot be had ends the creation, and the destructor frees those before it
        const size_t n = B;
        if ((e = arena_.alloc((size_t)a.bytes)) != hipSuccess || (e = h_counts_.alloc(sizeof(int) * n * L)) != hipSuccess ||
            (e = h_motion_.alloc(sizeof(double) * n * (3 + 7 * N))) != hipSuccess || (e = step_.alloc(step_bytes(B))) != hipSuccess ||
            (e = h_assess_.alloc(sizeof(mbavo_pairs_assessment) * n)) != hipSuccess || (e = h_keys_.alloc(sizeof(int) * n)) != hipSuccess ||
            (e = h_state_.alloc((size_t)a.span_bytes)) != hipSuccess || (e = h_times_.alloc(sizeof(double) * 3 * n)) != hipSuccess ||
            (e = h_frames_.alloc(sizeof(mbavo_pairs_frame) * n)) != hipSuccess ||
            (e = h_cams_.alloc(a.cams_bytes > 0 ? (size_t)a.cams_bytes : 8)) != hipSuccess) // (one camera for all pairs: a token allocation)
            return (int)e;
        memset(h_state_, 0, (size_t)a.span_bytes);
        hipStream_t st = eng_.stream();
        // deterministic contents for what a prepare does not write (pads) and for the motion before set_motion
        if ((e = hipMemsetAsync(arena_, 0, (size_t)a.bytes, st)) != hipSuccess) return (int)e;
        if ((e = hipMemsetAsync(step_, 0, step_bytes(B), st)) != hipSuccess) return (int)e;
        if (o->mask)
        { // no mask set yet: every pixel usable (the pads too).  A pinhole object waits for no camera call: its pyramids are built here
            if ((e = hipMemsetAsync(a.masks(arena_), 1, (size_t)p.mask_stride * (size_t)cameras(), st)) != hipSuccess) return (int)e;
            if (o->undistort == 0 && (rc = fill_clearance(cameras())) != 0) return rc;
        }

        std::vector<PairLevelDesc> desc((size_t)B * L);
        std::vector<const unsigned char *> cur_ptrs((size_t)B * L);
        std::vector<int> pattern(p.pat0[L]);
        for (int l = 0; l < L; ++l) memcpy(&pattern[p.pat0[l]], o->pattern_xy[l], sizeof(int) * 2 * o->P[l]);
        probs_.assign((size_t)B * L, mbavo_problem{});
        start_idx_.assign(B, 0);
        for (int b = 0; b < B; ++b)
            for (int l = 0; l < L; ++l)
            {
                const size_t e_ = (size_t)b * L + l;
                PairLevelDesc &d = desc[e_];
                d.ref = a.images(arena_) + (long long)b * p.img_stride + p.px0[l];
                d.cur = a.images(arena_) + (long long)(B + b) * p.img_stride + p.px0[l];
                d.grad = a.grad(arena_) + (long long)b * p.grad_stride + p.px0[l] * p.grad_bytes;
                d.kp_xy = a.keypoints(arena_) + (long long)b * p.kp_stride + p.kp0[l];
                d.kp_z = d.kp_xy + 2 * align_up(p.cap[l], 2);
                if (p.dense) d.seg = a.seg(arena_) + (long long)b * p.seg0[L] + p.seg0[l];
                else d.picks = a.picks(arena_) + (long long)b * p.cell0[L] + p.cell0[l];
                d.H = p.H[l]; d.W = p.W[l]; d.ch = p.ch[l]; d.cw = p.cw[l]; d.cells_w = p.cells_w[l]; d.cells = p.cells[l];
                d.border = o->border[l]; d.scale = std::pow(2, l);
                d.clear0 = (int)p.clear0[l]; // (< 2^31: at most 4/3 of 2^22 pixels and the levels' padding)
                cur_ptrs[e_] = d.cur;
                mbavo_problem &q = probs_[e_];
                q.S = o->S[l]; q.F = 1; q.K = 0; q.P = o->P[l]; q.N = N; q.H = d.H; q.W = d.W;
                q.d_ref_img = d.ref; q.d_ref_dIxy = (const float *)d.grad;
                q.d_cur_imgs = a.cur_ptrs(arena_) + e_;
                q.d_kp_xy = d.kp_xy; q.kp_stride = 2; q.d_kp_z = d.kp_z;
                q.d_pattern = a.pattern(arena_) + p.pat0[l];
                q.d_outlier = nullptr; q.num_bad = 0;
                // (a set of cameras: the pair's own, from set_cameras on)
                for (int i = 0; i < 4; ++i) q.intrinsics[i] = o->num_cameras > 0 ? 0.0 : o->intrinsics[i] / (double)(1 << l);
                q.d_cap_time = a.cap(arena_) + b; q.d_exp_time = a.exp(arena_) + b;
                q.d_knots_t = a.knots_t(arena_) + (size_t)b * 3 * N; q.d_knots_R = a.knots_R(arena_) + (size_t)b * 4 * N;
                q.h_start_idx = &start_idx_[b];
                q.huber_a = o->huber_a; q.grad_fp16 = p.format;
            }
        // (pageable sources: the copies are staged before the calls return; the synchronisation below covers the rest)
        if ((e = hipMemcpyAsync(a.desc(arena_), desc.data(), sizeof(PairLevelDesc) * desc.size(), hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        if ((e = hipMemcpyAsync(a.cur_ptrs(arena_), cur_ptrs.data(), sizeof(void *) * cur_ptrs.size(), hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        if ((e = hipMemcpyAsync(a.pattern(arena_), pattern.data(), sizeof(int) * pattern.size(), hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        return (int)hipStreamSynchronize(st);
    }

    DepthConv PairBatch::depth_conv() const
    {
        DepthConv c;
        c.fx = opts_.intrinsics[0]; c.fy = opts_.intrinsics[1]; c.cx = opts_.intrinsics[2]; c.cy = opts_.intrinsics[3];
        c.unit = opts_.depth_unit; c.max = opts_.depth_max;
        return c;
    }

    template <class Camera>
    int PairBatch::set_camera_with(const Camera *from, int (*fill_map)(Engine &, const Camera *, const double *, int, int, float *))
    {
        if (!arena_ || opts_.undistort == 0 || opts_.num_cameras > 0) return MBAVO_E_ARG;
        if (from && raw_size_fixed(from->H, from->W)) return MBAVO_E_ARG; // (the object holds vignettes of another raw size)
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        const int rc = fill_map(eng_, from, opts_.intrinsics, plan_.H[0], plan_.W[0], lay_.maps(arena_));
        if (rc != 0) return rc; // (a bad camera: nothing launched, the camera before it stays)
        raw_H_ = from->H; raw_W_ = from->W;
        // (kept for the points of the raw geometry: the kernel takes the camera by value)
        raw_cam_ = mbavo_pairs_camera{};
        raw_cam_.H = from->H; raw_cam_.W = from->W;
        memcpy(raw_cam_.intrinsics, from->intrinsics, sizeof(raw_cam_.intrinsics));
        memcpy(raw_cam_.dist, from->dist, sizeof(raw_cam_.dist));
        memcpy(raw_cam_.to_intrinsics, opts_.intrinsics, sizeof(raw_cam_.to_intrinsics));
        if constexpr (std::is_same_v<Camera, mbavo_camera_unified>) { raw_cam_.model = 2; raw_cam_.xi = from->xi; }
        else raw_cam_.model = 1;
        return fill_clearance(1);
    }

    int PairBatch::fill_clearance(int n)
    {
        if (!has_clearance()) return 0;
        const PairsPlan &p = plan_;
        ClearLevels lv;
        if (clear_levels(p.H[0], p.W[0], p.L, kAlign, lv) != 0) return MBAVO_E_ARG; // (the plan's levels: clear0, clear_stride)
        unsigned char *work = nullptr; // (radius 0: no box passes, no scratch)
        if (opts_.valid_radius > 0 && !(work = (unsigned char *)eng_.named_scratch(kClearWorkSlot, (size_t)p.clear_stride * (size_t)n)))
            return (int)hipErrorOutOfMemory;
        ClearSources src{};
        if (opts_.undistort != 0) { src.maps = lay_.maps(arena_); src.Hs = raw_H_; src.Ws = raw_W_; }
        if (opts_.mask) { src.masks = lay_.masks(arena_); src.mask_stride = p.mask_stride; }
        return clearance_enqueue(eng_, n, src, lv, opts_.valid_radius, lay_.clear(arena_), work);
    }

    // Everything is checked before anything is copied or launched.  The stored masks are the level-0 term of every later
    // fill_clearance: this call's and those of the camera calls.
    int PairBatch::set_masks(int geometry, int n, const unsigned char *d_masks)
    {
        const PairsPlan &p = plan_;
        if (!arena_ || !opts_.mask || n != cameras() || !d_masks || (geometry != 0 && geometry != 1)) return MBAVO_E_ARG;
        if (geometry == 1 && (opts_.undistort == 0 || camera_missing())) return MBAVO_E_ARG; // (no map to warp through)
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        unsigned char *stored = lay_.masks(arena_);
        const size_t npx0 = (size_t)p.H[0] * p.W[0];
        if (geometry == 0)
        {
            if ((e = hipMemcpy2DAsync(stored, (size_t)p.mask_stride, d_masks, npx0, npx0, (size_t)n, hipMemcpyDeviceToDevice, eng_.stream())) != hipSuccess)
                return (int)e;
        }
        else
        {
            const int rc = undistort_mask_enqueue(eng_, n, d_masks, raw_H_, raw_W_, lay_.maps(arena_), p.H[0], p.W[0], stored, p.mask_stride);
            if (rc != 0) return rc;
        }
        return fill_clearance(n);
    }
    int PairBatch::set_camera(const mbavo_camera_radtan *from) { return set_camera_with(from, undistort_map); }
    int PairBatch::set_camera(const mbavo_camera_unified *from) { return set_camera_with(from, undistort_map_unified); }

    // Everything is checked (into a scratch vector) before anything is copied or launched; then one copy of [MapCamera G |
    // PairCamera B] from the pinned mirror and, with maps to fill, one launch.  The mirror is rewritten only once the copy of the
    // set_cameras before has left it (an event; long past in any real use), so the call waits for nothing else.
    int PairBatch::set_cameras(int G, const mbavo_pairs_camera *h_cams, const int *h_camera_of_pair)
    {
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L;
        if (!arena_ || opts_.num_cameras == 0 || G != opts_.num_cameras || !h_cams || !h_camera_of_pair) return MBAVO_E_ARG;
        if (raw_size_fixed(h_cams[0].H, h_cams[0].W)) return MBAVO_E_ARG; // (the object holds vignettes of another raw size)
        std::vector<char> up((size_t)lay_.cams_bytes); // (the arena's camera arrays, which start at o_map_cams)
        MapCamera *mc = lay_.map_cameras(up.data(), lay_.o_map_cams);
        PairCamera *pc = lay_.pair_cameras(up.data(), lay_.o_map_cams);
        for (int g = 0; g < G; ++g)
        {
            if (!map_camera_of(h_cams[g], p.H[0], p.W[0], mc[g])) return MBAVO_E_ARG; // (to_intrinsics with fx or fy 0: rejected there)
            if (h_cams[g].H != h_cams[0].H || h_cams[g].W != h_cams[0].W) return MBAVO_E_ARG;
        }
        for (int b = 0; b < B; ++b)
        {
            const int g = h_camera_of_pair[b];
            if (g < 0 || g >= G) return MBAVO_E_ARG;
            const double *K = h_cams[g].to_intrinsics;
            pc[b].fx = K[0]; pc[b].fy = K[1]; pc[b].cx = K[2]; pc[b].cy = K[3];
            pc[b].cam = g; pc[b].pad = 0;
        }
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        if (cameras_set_ && (e = hipEventSynchronize(cams_copied_)) != hipSuccess) return (int)e;
        memcpy(h_cams_, up.data(), up.size());
        if ((e = hipMemcpyAsync(lay_.map_cameras(arena_), h_cams_, up.size(), hipMemcpyHostToDevice, eng_.stream())) != hipSuccess) return (int)e;
        if ((e = hipEventRecord(cams_copied_, eng_.stream())) != hipSuccess) return (int)e;
        if (opts_.undistort != 0)
        {
            const int rc = undistort_map_batch_enqueue(eng_, lay_.map_cameras(arena_), G, p.H[0], p.W[0], lay_.maps(arena_));
            if (rc != 0) return rc;
        }
        for (int b = 0; b < B; ++b)
            for (int l = 0; l < L; ++l)
            {
                double *K = probs_[(size_t)b * L + l].intrinsics;
                K[0] = pc[b].fx / (double)(1 << l); K[1] = pc[b].fy / (double)(1 << l);
                K[2] = pc[b].cx / (double)(1 << l); K[3] = pc[b].cy / (double)(1 << l);
            }
        raw_H_ = h_cams[0].H; raw_W_ = h_cams[0].W;
        cameras_set_ = true;
        if (opts_.undistort != 0) return fill_clearance(G);
        return 0;
    }

    bool PairBatch::camera_missing() const
    {
        return opts_.num_cameras > 0 ? !cameras_set_ : (opts_.undistort != 0 && raw_H_ == 0);
    }

    CameraSet PairBatch::camera_set() const
    {
        CameraSet cs;
        cs.of_pair = lay_.pair_cameras(arena_);
        cs.maps = lay_.maps(arena_);
        cs.map_floats = 2ll * plan_.H[0] * plan_.W[0];
        cs.Hs = raw_H_; cs.Ws = raw_W_;
        cs.unit = opts_.depth_unit; cs.max = opts_.depth_max;
        return cs;
    }

    template <class F>
    int PairBatch::with_camera(F &&f) const
    {
        const RawDepth raw{lay_.maps(arena_), raw_H_, raw_W_};
        if (has_clearance())
        { // the same four cameras with the clearance pyramid(s) behind off_clear (undistort = 0: those of undistort = 1, no map read)
            const unsigned char *clear = lay_.clear(arena_);
            if (opts_.num_cameras > 0)
                return opts_.undistort == 2 ? f(PairCameras<true, true>{camera_set(), {clear, plan_.clear_stride}})
                                            : f(PairCameras<false, true>{camera_set(), {clear, plan_.clear_stride}});
            if (opts_.undistort == 2) return f(OneCamera<RawDepth, Clearance>{depth_conv(), raw, Clearance{clear}});
            return f(OneCamera<NoRawDepth, Clearance>{depth_conv(), NoRawDepth{}, Clearance{clear}});
        }
        if (opts_.num_cameras > 0) // the pair's own intrinsics and, for raw-geometry depth maps, its camera's map
            return opts_.undistort == 2 ? f(PairCameras<true>{camera_set()}) : f(PairCameras<false>{camera_set()});
        if (opts_.undistort == 2) // raw-geometry depth maps, looked up through the object's map
            return f(OneCamera<RawDepth>{depth_conv(), raw});
        return f(OneCamera<NoRawDepth>{depth_conv(), NoRawDepth{}});
    }

    int PairBatch::set_points_geometry(int geometry)
    {
        if (!arena_ || (geometry != 0 && geometry != 1) || (geometry == 1 && opts_.undistort == 0)) return MBAVO_E_ARG;
        points_geometry_ = geometry;
        return 0;
    }

    template <class CAM, class F>
    int PairBatch::with_points_geometry(const CAM &cam, F &&f) const
    {
        if (points_geometry_ == 0) return f(cam); // (the instantiations of an object that never set a geometry)
        if constexpr (CAM::kCameraSet)
            return f(RawPoints<CAM, SetRawCameras>{cam, {lay_.map_cameras(arena_), cam.cs.of_pair, raw_H_, raw_W_}});
        else
        {
            OneRawCamera one;
            if (!map_camera_of(raw_cam_, one.cam)) return 0; // (set_camera accepted it: cannot fail; camera_missing() has been checked)
            one.Hs = raw_H_; one.Ws = raw_W_;
            return f(RawPoints<CAM, OneRawCamera>{cam, one});
        }
    }

    int PairBatch::level0(int n_key, const int *d_keys, const unsigned char *d_sharp, int n_cur, const unsigned char *d_blur, CallStats &s)
    {
        const PairsPlan &p = plan_;
        const int npx0 = p.H[0] * p.W[0];
        hipStream_t st = eng_.stream();
        const PairLevelDesc *desc = lay_.desc(arena_);
        if (photocal_.active) return level0_calibrated(n_key, d_keys, d_sharp, n_cur, d_blur, s); // (mbavo_pairs_set_photometric)
        if (opts_.undistort != 0)
        { // raw images: the new keyframes and the new current frames in one remap launch
            const dim3 grid((npx0 + 1023) / 1024, n_key + n_cur);
            ++s.launches;
            if (opts_.num_cameras == 0)
            {
                hipLaunchKernelGGL(k_pairs_remap_level0<SharedMap>, grid, dim3(256), 0, st, desc, p.L, d_keys, n_key, d_sharp, d_blur, raw_H_, raw_W_,
                                   SharedMap{lay_.maps(arena_)}, npx0);
                return 0;
            }
            const CameraSet cs = camera_set();
            const CameraMaps maps{cs.maps, cs.of_pair, cs.map_floats};
            if (remap_both_ && !d_keys && n_key == p.B && n_cur == p.B) // a prepare: every pair brings both images
                hipLaunchKernelGGL(k_pairs_remap_level0_both, dim3(grid.x, p.B), dim3(256), 0, st, desc, p.L, d_sharp, d_blur, raw_H_, raw_W_, maps, npx0);
            else
                hipLaunchKernelGGL(k_pairs_remap_level0<CameraMaps>, grid, dim3(256), 0, st, desc, p.L, d_keys, n_key, d_sharp, d_blur, raw_H_, raw_W_,
                                   maps, npx0);
            return 0;
        }
        // one strided copy per image array into pairs 0 .. n - 1; the keyframes of a list through a kernel
        unsigned char *img = lay_.images(arena_);
        hipError_t e = hipSuccess;
        if (n_key > 0 && d_keys)
        {
            hipLaunchKernelGGL(k_pairs_scatter_level0, dim3((npx0 + 4095) / 4096, n_key), dim3(256), 0, st, desc, p.L, d_keys, d_sharp, npx0);
            ++s.launches;
        }
        else if (n_key > 0)
            e = hipMemcpy2DAsync(img, (size_t)p.img_stride, d_sharp, (size_t)npx0, (size_t)npx0, n_key, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess && n_cur > 0)
            e = hipMemcpy2DAsync(img + (size_t)p.B * p.img_stride, (size_t)p.img_stride, d_blur, (size_t)npx0, (size_t)npx0, n_cur, hipMemcpyDeviceToDevice, st);
        return (int)e;
    }

    // (d_depth: B maps in the object's depth format -- float z, float ray distance or uint16)
    int PairBatch::prepare(const unsigned char *d_sharp, const void *d_depth, const unsigned char *d_blur, int *h_counts)
    {
        if (!d_depth) return MBAVO_E_ARG;
        KeypointSource src;
        src.d_depth = d_depth;
        return prepare_from(d_sharp, d_blur, src, h_counts);
    }

    int PairBatch::prepare_points(const unsigned char *d_sharp, const unsigned char *d_blur, const int *h_offsets, const double *d_xy,
                                  const double *d_z, int *h_counts)
    {
        KeypointSource src;
        src.points = true; src.h_offsets = h_offsets; src.d_xy = d_xy; src.d_z = d_z;
        return prepare_from(d_sharp, d_blur, src, h_counts);
    }

    // Pure host, on the offsets alone: a row longer than the smallest capacity of the levels could overrun that level's slice.
    int PairBatch::check_points(int rows, const int *h_offsets, const double *d_xy, const double *d_z) const
    {
        if (!h_offsets || h_offsets[0] != 0) return MBAVO_E_ARG;
        for (int i = 0; i < rows; ++i)
            if (h_offsets[i + 1] < h_offsets[i]) return MBAVO_E_ARG;
        if (h_offsets[rows] > 0 && (!d_xy || !d_z)) return MBAVO_E_ARG;
        int cap = plan_.cap[0];
        for (int l = 1; l < plan_.L; ++l) cap = plan_.cap[l] < cap ? plan_.cap[l] : cap;
        for (int i = 0; i < rows; ++i)
            if (h_offsets[i + 1] - h_offsets[i] > cap) return MBAVO_E_RANGE;
        return 0;
    }

    const int *PairBatch::upload_offsets(int rows, const int *h_offsets)
    { // (a pageable source: the copy is staged before the call returns; create has reserved B + 1 ints, so nothing grows here)
        int *d = (int *)eng_.named_scratch(kPointOffsetsSlot, sizeof(int) * ((size_t)plan_.B + 1));
        if (!d || hipMemcpyAsync(d, h_offsets, sizeof(int) * ((size_t)rows + 1), hipMemcpyHostToDevice, eng_.stream()) != hipSuccess) return nullptr;
        return d;
    }

    int PairBatch::prepare_from(const unsigned char *d_sharp, const unsigned char *d_blur, KeypointSource src, int *h_counts)
    {
        if (!arena_ || !d_sharp || !d_blur) return MBAVO_E_ARG;
        if (camera_missing()) return MBAVO_E_ARG; // (no camera yet)
        const int B = plan_.B, L = plan_.L;
        if (src.points)
        {
            const int rc = check_points(B, src.h_offsets, src.d_xy, src.d_z);
            if (rc != 0) return rc;
        }
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        if (src.points && !(src.d_offsets = upload_offsets(B, src.h_offsets))) return (int)hipErrorOutOfMemory;
        stats_ = CallStats{};
        const int rc = refresh(B, nullptr, d_sharp, B, d_blur, src, stats_); // an update of everything, without a list
        if (rc != 0) return rc;
        kp_serial_.resize(B, 0);
        for (int b = 0; b < B; ++b) ++kp_serial_[b]; // (every pair's keypoints are rewritten: the depth filter seeds them anew)
        if (h_counts) memcpy(h_counts, h_counts_, sizeof(int) * B * L);
        prepared_ = true;
        return 0;
    }

    int PairBatch::read_back(const void *d_src, void *h_mirror, void *h_out, size_t bytes, CallStats &s)
    {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        if (bytes > 0 && (e = hipMemcpyAsync(h_mirror, d_src, bytes, hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
        s.bytes_back = (long long)bytes;
        e = hipStreamSynchronize(st);
        s.syncs = 1;
        if (e != hipSuccess) return (int)e;
        if (h_out && bytes > 0) memcpy(h_out, h_mirror, bytes);
        return 0;
    }

    DepthSlots::DepthSlots(const PairsPlan &p)
    {
        for (int l = 0; l < p.L; ++l)
        {
            groups256[l] = groups(p.cap[l], 256);
            st0[l + 1] = st0[l] + p.cap[l];
        }
        st_stride = st0[p.L];
        n_slots = (size_t)p.B * (size_t)st_stride;
    }

    int DepthSlots::groups(long long cap, int T)
    {
        const long long tiles = (cap + T - 1) / T;
        return tiles < 1 ? 1 : (tiles < kRefineGroups ? (int)tiles : kRefineGroups);
    }

    long long DepthSlots::outs(int level, long long out0[8]) const
    {
        for (int l = 0; l < 8; ++l) out0[l] = level < 0 && groups256[l] > 0 ? st0[l] : 0; // (no workgroups: past the last level)
        return level < 0 ? st_stride : st0[level + 1] - st0[level];
    }

    int DepthSlots::width(int level, const int g[8])
    { // (g is zero past the last level)
        int w = 1;
        for (int l = 0; l < 8; ++l)
            if ((level < 0 || level == l) && g[l] > w) w = g[l];
        return w;
    }

    hipError_t DepthCall::open(size_t rec_bytes_max, int sums, size_t opt_bytes, int levels)
    {
        const int B = pb.plan_.B, L = levels > 0 ? levels : pb.plan_.L;
        hipStream_t st = pb.eng_.stream();
        hipError_t e;
        const long long o_parts = align_up((long long)rec_bytes_max, kAlign);
        const long long o_tickets = o_parts + align_up((long long)sizeof(double) * sums * kRefineGroups * B * L, kAlign);
        const long long o_opts = o_tickets + align_up((long long)sizeof(int) * B * L, kAlign);
        if (!dev)
        { // (the tickets start at zero; the last workgroup of a (pair, level) leaves its ticket at zero again)
            if ((e = dev.alloc((size_t)o_opts + opt_bytes)) != hipSuccess) return e;
            if ((e = hipMemsetAsync(dev + o_tickets, 0, sizeof(int) * (size_t)B * L, st)) != hipSuccess) return e;
        }
        if (!mirror && (e = mirror.alloc(rec_bytes_max + opt_bytes)) != hipSuccess) return e;
        if (copied) e = hipEventSynchronize(copied); // (an earlier call that waited for nothing may still be reading the mirror)
        else if ((e = hipEventCreateWithFlags(&copied, hipEventDisableTiming)) != hipSuccess) copied = nullptr;
        if (e != hipSuccess) return e;
        records = dev.p;
        partials = (double *)(dev + o_parts); tickets = (int *)(dev + o_tickets);
        d_opts = dev + o_opts; h_opts = mirror + rec_bytes_max;
        return hipSuccess;
    }

    hipError_t DepthCall::upload(size_t bytes)
    {
        hipStream_t st = pb.eng_.stream();
        const hipError_t e = hipMemcpyAsync(d_opts, h_opts, bytes, hipMemcpyHostToDevice, st);
        return e != hipSuccess ? e : hipEventRecord(copied, st);
    }

    int DepthCall::finish(void *h_out, size_t rec_bytes, CallStats *st)
    {
        if (!h_out) return (int)hipGetLastError(); // (nothing is waited for)
        return pb.read_back(records, mirror, h_out, rec_bytes, st ? *st : stats);
    }

    void PairBatch::pyramids(int n_key, const int *d_keys, int n_cur, CallStats &s)
    {
        const PairsPlan &p = plan_;
        const int L = p.L;
        for (int l = 0; l + 1 < L; l += 3)
        {
            const int n = L - 1 - l < 3 ? L - 1 - l : 3;
            hipLaunchKernelGGL(k_pairs_pyr_down, dim3((p.W[l] / 2 + 15) / 16, (p.H[l] / 2 + 15) / 16, n_key + n_cur), dim3(256), 0, eng_.stream(),
                               lay_.desc(arena_), d_keys, n_key, L, l, n);
            ++s.launches;
        }
    }

    // What a prepare and an update share: see pairs_prep.h.  (n_key == 0: no keyframe launch, no count copy.)
    int PairBatch::refresh(int n_key, const int *d_keys, const unsigned char *d_sharp, int n_cur, const unsigned char *d_blur,
                           const KeypointSource &src, CallStats &s)
    {
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L;
        hipStream_t st = eng_.stream();
        const PairLevelDesc *desc = lay_.desc(arena_);
        int *d_counts = lay_.counts(arena_);
        const int rc = level0(n_key, d_keys, d_sharp, n_cur, d_blur, s);
        if (rc != 0) return rc;
        pyramids(n_key, d_keys, n_cur, s);
        if (n_key > 0)
        {
            const PairsGrid g = pairs_grid(p);
            const dim3 ggrid(g.blk0[L], n_key);
            if (p.format == 0) hipLaunchKernelGGL(k_pairs_gradients<0>, ggrid, dim3(256), 0, st, desc, g, d_keys);
            else if (p.format == 1) hipLaunchKernelGGL(k_pairs_gradients<1>, ggrid, dim3(256), 0, st, desc, g, d_keys);
            else hipLaunchKernelGGL(k_pairs_gradients<2>, ggrid, dim3(256), 0, st, desc, g, d_keys);
            ++s.launches;
            const bool scored = detector_.score != 0 && !src.points; // (mbavo_pairs_set_detector; the caller's points have no detector)
            if (scored) score_levels(n_key, d_keys, s);
            s.launches += with_camera([&](const auto &cam) {
                if (src.points)
                    return with_points_geometry(cam, [&](const auto &pcam) { return launch_points(p, st, desc, d_counts, n_key, d_keys, src, pcam); });
                if (scored)
                    return launch_keypoints(opts_.depth_format, p, g, st, desc, d_counts, detector_.threshold, src.d_depth, n_key, d_keys,
                                            ScoredCamera<std::decay_t<decltype(cam)>>{cam, score_slices()});
                return launch_keypoints(opts_.depth_format, p, g, st, desc, d_counts, opts_.score_threshold, src.d_depth, n_key, d_keys, cam);
            });
        }
        // (the counts only where keyframes changed; the synchronisation always: the caller's images are free again)
        const int rb = read_back(d_counts, h_counts_, nullptr, n_key > 0 ? sizeof(int) * B * L : 0, s);
        if (rb != 0) return rb;
        if (n_key > 0)
            for (int i = 0; i < B * L; ++i) probs_[i].K = h_counts_[i]; // (the pairs not listed: their counts as they were)
        return 0;
    }

    bool PairBatch::samples_on_knots(const double *h_cap, const double *h_exp, const double *h_t0, double dt) const
    { // the kernels' own sample times (compute_virtual_camera_poses.cu:33), checked on the host as the host-driven tracker does
        for (int b = 0; b < plan_.B; ++b)
        {
            const double t0 = h_t0 ? h_t0[b] : h_cap[b] - 0.5 * h_exp[b]; // (blur_aware_direct_tracker.cpp:131 setStartTime)
            for (int l = 0; l < plan_.L; ++l)
                for (int smp = 0; smp < opts_.S[l]; ++smp)
                {
                    const double ts = h_cap[b] - h_exp[b] * 0.5 + smp * h_exp[b] / (opts_.S[l] - 1 + 1e-8);
                    int idx;
                    double u;
                    if (!spline_segment_checked(ts, t0, dt, plan_.N, opts_.spline_deg_k, idx, u)) return false;
                }
        }
        return true;
    }

    void PairBatch::publish_times(const double *h_cap, const double *h_t0, double dt)
    {
        const int B = plan_.B, L = plan_.L;
        for (int b = 0; b < B; ++b)
        {
            start_idx_[b] = spline_segment_index(h_cap[b], h_t0[b], dt); // mbavo_segment_start_index
            for (int l = 0; l < L; ++l)
            {
                probs_[(size_t)b * L + l].t0 = h_t0[b];
                probs_[(size_t)b * L + l].dt = dt;
            }
        }
    }

    int PairBatch::set_motion(const double *h_cap, const double *h_exp, const double *h_t0, double dt, const double *h_kt, const double *h_kR)
    {
        if (!arena_ || !h_cap || !h_exp || !h_t0 || !h_kt || !h_kR || !(dt > 0)) return MBAVO_E_ARG;
        const int B = plan_.B, N = plan_.N;
        if (!samples_on_knots(h_cap, h_exp, h_t0, dt)) return MBAVO_E_RANGE; // (nothing is touched before every pair has passed)
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
        if ((e = hipMemcpyAsync(lay_.cap(arena_), m, sizeof(double) * B * (2 + 7 * N), hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        if ((e = hipMemcpyAsync(lay_.t0(arena_), m_t0, sizeof(double) * B, hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return (int)e; // (the staging buffer is free again)
        motion_set_ = true;
        publish_times(h_cap, h_t0, dt);
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
        if ((e = hipMemcpyAsync(h_motion_ + first, lay_.knots_t(arena_), n * sizeof(double), hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return (int)e;
        memcpy(h_kt, h_motion_ + first, sizeof(double) * B * 3 * N);
        memcpy(h_kR, h_motion_ + first + (size_t)B * 3 * N, sizeof(double) * B * 4 * N);
        return 0;
    }

    int PairBatch::update(const unsigned char *d_blur, int n_key, const int *h_key_pairs, const unsigned char *d_sharp, const void *d_depth, int *h_counts)
    {
        if (n_key > 0 && !d_depth) return MBAVO_E_ARG;
        KeypointSource src;
        src.d_depth = d_depth;
        return update_from(d_blur, n_key, h_key_pairs, d_sharp, src, h_counts);
    }

    int PairBatch::update_points(const unsigned char *d_blur, int n_key, const int *h_key_pairs, const unsigned char *d_sharp, const int *h_offsets,
                                 const double *d_xy, const double *d_z, int *h_counts)
    {
        KeypointSource src;
        src.points = n_key > 0; // (no keyframe, no list: mbavo_pairs_update(d_blur, 0, ..), the point arguments are not read)
        src.h_offsets = h_offsets; src.d_xy = d_xy; src.d_z = d_z;
        return update_from(d_blur, n_key, h_key_pairs, d_sharp, src, h_counts);
    }

    int PairBatch::update_from(const unsigned char *d_blur, int n_key, const int *h_key_pairs, const unsigned char *d_sharp, KeypointSource src,
                               int *h_counts)
    {
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L;
        if (!arena_ || !prepared_ || n_key < 0 || n_key > B) return MBAVO_E_ARG;
        if (camera_missing()) return MBAVO_E_ARG; // (no camera yet; a prepare needs one too)
        if (n_key > 0 && (!h_key_pairs || !d_sharp)) return MBAVO_E_ARG;
        for (int i = 0; i < n_key; ++i)
            if (h_key_pairs[i] < 0 || h_key_pairs[i] >= B || (i > 0 && h_key_pairs[i] <= h_key_pairs[i - 1])) return MBAVO_E_ARG;
        if (src.points)
        {
            const int rc = check_points(n_key, src.h_offsets, src.d_xy, src.d_z);
            if (rc != 0) return rc;
        }
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        if (src.points && !(src.d_offsets = upload_offsets(n_key, src.h_offsets))) return (int)hipErrorOutOfMemory;
        const int *d_keys = (const int *)(step_ + step_off_keys(B));
        upd_stats_ = CallStats{};
        const int n_cur = d_blur ? B : 0;
        if (n_key + n_cur > 0)
        { // (else nothing changes)
            if (n_key > 0)
            {
                memcpy(h_keys_, h_key_pairs, sizeof(int) * n_key);
                if ((e = hipMemcpyAsync((void *)d_keys, h_keys_, sizeof(int) * n_key, hipMemcpyHostToDevice, eng_.stream())) != hipSuccess) return (int)e;
            }
            const int rc = refresh(n_key, d_keys, d_sharp, n_cur, d_blur, src, upd_stats_); // (row y of the source belongs to pair key_pairs[y])
            if (rc != 0) return rc;
            for (int i = 0; i < n_key; ++i) ++kp_serial_[h_key_pairs[i]]; // (their keypoints are rewritten: the depth filter seeds them anew)
        }
        if (h_counts) for (int i = 0; i < B * L; ++i) h_counts[i] = probs_[i].K;
        return 0;
    }

    void PairBatch::last_stats(long long out[4]) const
    {
        stats_.get(out);
        out[3] = arena_ ? plan_.total : 0;
    }
} // namespace mbavo

// keyframe_ops.hip -- keyframe pre-processing on device: gradient magnitude, semi-dense
// keypoint selection and the depth lookup of BlurAwareDirectTracker::tmpProcessKeyframe, so that a new keyframe
// needs one H2D of the image (+ depth map) and one small D2H of the keypoint count instead of host loops over
// every pixel of every level.
//
//   gradient magnitude   core/image_proc/Gradient.h:56-71       sqrt(dx^2 + dy^2) of the central differences
//   candidates           FeatureDetectorSemiDense.cpp:27-43      magnitude > score_threshold, row-major order
//   grid selection       FeatureDetectorBase.cpp:49-91           per cell the first pixel of strictly largest response
//   depth lookup         blur_aware_direct_tracker.cpp:389-415   z at the level-0 position, drop z < 1e-2
//
// Integer / index work: results (positions, order, count) are bit-identical to the CPU restatement.
// The magnitude is never materialised for the detector: it is recomputed from the u8 image (3 loads per pixel,
// L2-resident), which is cheaper than writing and re-reading a float image.  One wave per grid cell; the ordered
// compaction over <= a few thousand cells is a single-block scan.  HBM-bound streaming work, ~1 byte per pixel.
//
// The kernels here find their image, level, cell or row; the pyramid tile, the pixel's differences, the wave's scan of a cell and
// the workgroup prefix sums they call are keyframe_math.h's, as are the batched kernels' (pairs_prep.hip).  cell_grid is the one
// place where a level's grid is laid out, for both.
#include "../../include/mbavo.h"
#include "engine.h"
#include "keyframe_math.h"
#include "vo_frontend.h"
#include <cmath>
#include <cstring>
#include <hip/hip_runtime.h>
#include <vector>

namespace mbavo
{
    __global__ void k_grad_mag(const unsigned char *__restrict__ src, int H, int W, float *__restrict__ mag)
    {
        const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
        if (x >= W || y >= H) return;
        mag[(size_t)y * W + x] = gradient_magnitude(src, H, W, x, y);
    }

    // one wave per grid cell
    __device__ __forceinline__ void detect_cell(const unsigned char *__restrict__ src, int H, int W, int cell_h, int cell_w, int cells_w,
                                                float thr, const float *__restrict__ depth, int W0, double scale, int ci, int lane,
                                                CellPick *__restrict__ picks)
    {
        float best;
        int best_idx;
        best_pixel_in_cell(src, H, W, (ci / cells_w) * cell_h, (ci % cells_w) * cell_w, cell_h, cell_w, thr, lane, best, best_idx);
        if (lane == 0)
        {
            CellPick p = pick_at(best, best_idx, W);
            if (p.keep && depth != nullptr) p.keep = depth_of(depth, W0, scale, p.x, p.y, p.z) ? 1 : 0; // (null: the caller tests the depth)
            picks[ci] = p;
        }
    }
    __global__ __launch_bounds__(64) void k_detect_cells(const unsigned char *__restrict__ src, int H, int W, int cell_h,
                                                         int cell_w, int cells_w, float thr,
                                                         const float *__restrict__ depth, int W0, double scale,
                                                         CellPick *__restrict__ picks)
    {
        detect_cell(src, H, W, cell_h, cell_w, cells_w, thr, depth, W0, scale, (int)blockIdx.x, (int)threadIdx.x, picks);
    }

    // ---- a keyframe's levels in ONE launch each (round 3): the per-level kernels are latency-bound (4-10 us each whatever the
    // level's size), and a keyframe ran 3 of them per level back to back -- 11 launches at four levels, ~100 us of the 150 us a
    // keyframe cost.  The levels' parameters travel by value; a workgroup finds its level from the prefix sums.
    struct PyramidLevels
    {
        const unsigned char *img[8];
        float2 *grad[8];
        int H[8], W[8];
        int row0[9];                         // gradients: first grid row of every level
        int ch[8], cw[8], cells_w[8], cell0[9]; // grid selection: cell size, cells per row, first cell of every level
        double scale[8];
        int n;
    };
    // up to three levels below `src` in one launch, a 32 x 32 source tile per workgroup (keyframe_math.h: pyr_down_tile)
    __global__ __launch_bounds__(256) void k_pyr_down_multi(const unsigned char *__restrict__ src, int Hs, int Ws, unsigned char *__restrict__ d1,
                                                            unsigned char *__restrict__ d2, unsigned char *__restrict__ d3, int n)
    {
        pyr_down_tile(src, Hs, Ws, d1, d2, d3, n);
    }
    // interleaved [dx, dy] central differences of every level (what image_ops.hip's k_gradients<0> stores)
    __global__ __launch_bounds__(256) void k_gradients_multi(const PyramidLevels lv)
    {
        int l = 0;
        while (l + 1 < lv.n && (int)blockIdx.y >= lv.row0[l + 1]) ++l;
        const int H = lv.H[l], W = lv.W[l], y = (int)blockIdx.y - lv.row0[l], x = blockIdx.x * blockDim.x + threadIdx.x;
        if (x >= W || y >= H) return;
        const size_t i = (size_t)y * W + x;
        int kx, ky;
        central_diff(lv.img[l], H, W, x, y, i, kx, ky);
        lv.grad[l][i] = GradPixel<0>::of(0, kx, ky);
    }
    // grid selection of every level: one wave per cell, the cells of all levels in one grid (picks in level order)
    __global__ __launch_bounds__(64) void k_detect_cells_multi(const PyramidLevels lv, float thr, int W0, CellPick *__restrict__ picks)
    {
        int l = 0;
        while (l + 1 < lv.n && (int)blockIdx.x >= lv.cell0[l + 1]) ++l;
        detect_cell(lv.img[l], lv.H[l], lv.W[l], lv.ch[l], lv.cw[l], lv.cells_w[l], thr, nullptr, W0, lv.scale[l],
                    (int)blockIdx.x - lv.cell0[l], (int)threadIdx.x, picks + lv.cell0[l]);
    }

    // ordered compaction of the kept cells: single block, 256 cells per step
    __global__ __launch_bounds__(256) void k_compact_cells(const CellPick *__restrict__ picks, int n, double *__restrict__ kp_xy,
                                                           double *__restrict__ kp_z, int cap, int *__restrict__ count)
    {
        __shared__ int wave_total[4];
        int base = 0;
        for (int c0 = 0; c0 < n; c0 += 256)
        {
            const int i = c0 + (int)threadIdx.x;
            CellPick p;
            p.keep = 0;
            if (i < n) p = picks[i];
            int total;
            const int pos = base + block_rank_of_flag(p.keep != 0, wave_total, total);
            if (p.keep && pos < cap)
            {
                kp_xy[2 * pos] = (double)p.x; kp_xy[2 * pos + 1] = (double)p.y;
                kp_z[pos] = (double)p.z;
            }
            base += total;
            __syncthreads(); // (wave_total is rewritten in the next step)
        }
        if (threadIdx.x == 0) *count = base;
    }

    // ---- no grid selection: every candidate, in row-major order.  Rows are the segments of the ordered compaction.
    __device__ __forceinline__ bool row_candidate(const unsigned char *__restrict__ src, int H, int W, float thr,
                                                  const float *__restrict__ depth, int W0, double scale, int x, int y, float &z)
    {
        if (x >= W) return false;
        const float m = gradient_magnitude(src, H, W, x, y);
        if (!(m > thr)) return false;
        return depth_of(depth, W0, scale, x, y, z);
    }

    __global__ __launch_bounds__(64) void k_rows_count(const unsigned char *__restrict__ src, int H, int W, float thr,
                                                       const float *__restrict__ depth, int W0, double scale,
                                                       int *__restrict__ row_count)
    {
        const int y = blockIdx.x, lane = threadIdx.x;
        int n = 0;
        for (int x0 = 0; x0 < W; x0 += 64)
        {
            float z;
            n += __popcll(__ballot(row_candidate(src, H, W, thr, depth, W0, scale, x0 + lane, y, z)));
        }
        if (lane == 0) row_count[y] = n;
    }

    __global__ __launch_bounds__(256) void k_rows_scan(int *__restrict__ row_count, int H, int *__restrict__ count)
    { // in-place exclusive scan over the rows, 256 per step
        __shared__ int wave_total[4];
        int base = 0;
        for (int c0 = 0; c0 < H; c0 += 256)
        {
            const int i = c0 + (int)threadIdx.x;
            int total;
            const int before = block_exclusive_scan(i < H ? row_count[i] : 0, wave_total, total);
            if (i < H) row_count[i] = base + before;
            base += total;
            __syncthreads(); // (wave_total is rewritten in the next step)
        }
        if (threadIdx.x == 0) *count = base;
    }

    __global__ __launch_bounds__(64) void k_rows_write(const unsigned char *__restrict__ src, int H, int W, float thr,
                                                       const float *__restrict__ depth, int W0, double scale,
                                                       const int *__restrict__ row_off, double *__restrict__ kp_xy,
                                                       double *__restrict__ kp_z, int cap)
    {
        const int y = blockIdx.x, lane = threadIdx.x;
        int pos = row_off[y];
        for (int x0 = 0; x0 < W; x0 += 64)
        {
            float z = 0.f;
            const bool c = row_candidate(src, H, W, thr, depth, W0, scale, x0 + lane, y, z);
            const unsigned long long b = __ballot(c);
            const int mine = pos + __popcll(b & ((1ull << lane) - 1ull));
            if (c && mine < cap)
            {
                kp_xy[2 * mine] = (double)(x0 + lane); kp_xy[2 * mine + 1] = (double)y;
                kp_z[mine] = (double)z;
            }
            pos += __popcll(b);
        }
    }

    int cell_grid(int H0, int W0, int level, int cell_H, int cell_W, int H, int W, CellGrid &g)
    { // FeatureDetectorBase.cpp:56-64
        const int sf = (int)std::pow(2, level);
        const int Hl = H0 / sf, Wl = W0 / sf;
        g.ch = (int)(cell_H / std::pow(1.414, level)); g.cw = (int)(cell_W / std::pow(1.414, level));
        if (g.ch < 1 || g.cw < 1) return MBAVO_E_ARG; // the reference divides by zero here
        g.cells_h = Hl / g.ch + 1; g.cells_w = Wl / g.cw + 1;
        if ((H - 1) / g.ch >= g.cells_h || (W - 1) / g.cw >= g.cells_w) return MBAVO_E_RANGE; // std::vector::at would throw
        return 0;
    }

    int detect_semidense(Engine &eng, const unsigned char *d_img, int H, int W, int level, int im_H0, int im_W0, int cell_H,
                         int cell_W, float thr, const float *d_depth_z, double *d_kp_xy, double *d_kp_z, int cap, int *h_count)
    {
        if (!d_img || !d_depth_z || !d_kp_xy || !d_kp_z || !h_count || H < 1 || W < 1 || level < 0 || level > 30 || cap < 0)
            return MBAVO_E_ARG;
        hipStream_t st = eng.stream();
        const double scale = std::pow(2, level);
        int *d_count = (int *)eng.named_scratch(kKeypointCountSlot, sizeof(int));
        if (!d_count) return MBAVO_E_ARG;
        hipError_t e;
        if (cell_H > 0 && cell_W > 0)
        {
            CellGrid g;
            const int rc = cell_grid(im_H0, im_W0, level, cell_H, cell_W, H, W, g);
            if (rc != 0) return rc;
            const int nc = g.cells_h * g.cells_w;
            CellPick *picks = (CellPick *)eng.named_scratch(kCellWorkSlot, sizeof(CellPick) * nc);
            if (!picks) return MBAVO_E_ARG;
            hipLaunchKernelGGL(k_detect_cells, dim3(nc), dim3(64), 0, st, d_img, H, W, g.ch, g.cw, g.cells_w, thr, d_depth_z, im_W0, scale, picks);
            hipLaunchKernelGGL(k_compact_cells, dim3(1), dim3(256), 0, st, picks, nc, d_kp_xy, d_kp_z, cap, d_count);
        }
        else
        {
            int *rows = (int *)eng.named_scratch(kCellWorkSlot, sizeof(int) * H);
            if (!rows) return MBAVO_E_ARG;
            hipLaunchKernelGGL(k_rows_count, dim3(H), dim3(64), 0, st, d_img, H, W, thr, d_depth_z, im_W0, scale, rows);
            hipLaunchKernelGGL(k_rows_scan, dim3(1), dim3(256), 0, st, rows, H, d_count);
            hipLaunchKernelGGL(k_rows_write, dim3(H), dim3(64), 0, st, d_img, H, W, thr, d_depth_z, im_W0, scale, rows, d_kp_xy, d_kp_z, cap);
        }
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        if ((e = hipMemcpyAsync(h_count, d_count, sizeof(int), hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
        return (int)hipStreamSynchronize(st);
    }

    // ---- a whole depth map to float z: every pixel through the body the detectors use for the pixels they look up
    template <int FORMAT>
    __global__ __launch_bounds__(256) void k_depth_to_z(const typename DepthMap<FORMAT>::elem *__restrict__ map, int W, unsigned npx,
                                                        const DepthConv dc, float *__restrict__ z)
    { // (npx < 2^31: the flat index and its division stay in 32 bits)
        const unsigned i = blockIdx.x * 256u + threadIdx.x;
        if (i >= npx) return;
        const unsigned y = i / (unsigned)W, x = i - y * (unsigned)W;
        z[i] = depth_z_at<FORMAT>(map, W, (int)x, (int)y, dc);
    }

    int depth_to_z(Engine &eng, int depth_format, const void *d_depth, int H, int W, const double intrinsics[4], float depth_unit,
                   float depth_max, float *d_z)
    {
        if (!depth_format_valid(depth_format, depth_unit) || !d_depth || !d_z || !intrinsics || H < 1 || W < 1) return MBAVO_E_ARG;
        if ((long long)H * W > 0x7fffffffll) return MBAVO_E_ARG;
        const unsigned npx = (unsigned)H * (unsigned)W, blocks = (npx + 255u) / 256u;
        DepthConv dc;
        dc.fx = intrinsics[0]; dc.fy = intrinsics[1]; dc.cx = intrinsics[2]; dc.cy = intrinsics[3];
        dc.unit = depth_unit; dc.max = depth_max;
        hipStream_t st = eng.stream();
        const dim3 grid(blocks);
        if (depth_format == 0) hipLaunchKernelGGL(k_depth_to_z<0>, grid, dim3(256), 0, st, (const float *)d_depth, W, npx, dc, d_z);
        else if (depth_format == 1) hipLaunchKernelGGL(k_depth_to_z<1>, grid, dim3(256), 0, st, (const float *)d_depth, W, npx, dc, d_z);
        else hipLaunchKernelGGL(k_depth_to_z<2>, grid, dim3(256), 0, st, (const unsigned short *)d_depth, W, npx, dc, d_z);
        return (int)hipGetLastError();
    }

    // ---- images of a camera with lens distortion (camera_math.h; include/mbavo.h: mbavo_undistort_map, _map_unified, _u8, _u8_batch).
    // The map: two adjacent pixels of the flat H*W image per lane, stored as 16 bytes where the caller's buffer allows it.
    // Cams: UndistortCams (pinhole + radial-tangential) or UndistortCamsUnified -- the camera model picks the entry's overload.
    // undistort_map_two is the body of both kernels, the single camera's and the batch's.
    template <class Cams>
    __device__ __forceinline__ void undistort_map_two(const Cams &m, int W, int npx, float *__restrict__ map)
    {
        const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 2;
        if (i0 >= npx) return;
        int r = i0 / W, c = i0 - r * W;
        const float2 a = undistort_map_entry(m, c, r);
        float *out = map + 2 * (size_t)i0;
        if (i0 + 1 >= npx)
        { // an odd pixel count: the last lane has one pixel
            out[0] = a.x; out[1] = a.y;
            return;
        }
        if (++c == W) { c = 0; ++r; }
        const float2 b = undistort_map_entry(m, c, r);
        if (((size_t)out & 15) == 0) *reinterpret_cast<float4 *>(out) = make_float4(a.x, a.y, b.x, b.y);
        else { out[0] = a.x; out[1] = a.y; out[2] = b.x; out[3] = b.y; }
    }
    template <class Cams>
    __global__ __launch_bounds__(256) void k_undistort_map(const Cams m, int W, int npx, float *__restrict__ map)
    {
        undistort_map_two(m, W, npx, map);
    }
    // The maps of n cameras in one launch: camera blockIdx.y of a device array, its map at float 2 * npx * blockIdx.y (16-byte
    // aligned or not: the store above looks).  The camera's fields are the same for the whole workgroup (scalar loads), and so is
    // the branch on its model; each side is the entry function of the single-camera kernel, so the bits are that kernel's.
    __global__ __launch_bounds__(256) void k_undistort_map_batch(const MapCamera *__restrict__ cams, int W, int npx, float *__restrict__ maps)
    {
        const MapCamera &cam = cams[blockIdx.y];
        float *__restrict__ map = maps + 2 * (size_t)npx * blockIdx.y;
        if (cam.model == 2) undistort_map_two(cam.u, W, npx, map);
        else undistort_map_two(cam.u.c, W, npx, map);
    }
    // Raw points into the undistorted images of n cameras in one launch (include/mbavo.h: mbavo_undistort_points_batch): grid row
    // blockIdx.y takes points offsets[y] .. offsets[y + 1] - 1 through camera y, a lane one point (camera_math.h:
    // undistorted_position, the function the pairs batch calls).  The grid is as wide as the longest row; the workgroups past a
    // row's end leave at once.  The camera's fields are the same for the whole workgroup (scalar loads).
    __global__ __launch_bounds__(256) void k_undistort_points_batch(const MapCamera *__restrict__ cams, const int *__restrict__ offsets,
                                                                    const double *__restrict__ uv, double *__restrict__ xy,
                                                                    unsigned char *__restrict__ ok)
    {
        const int first = offsets[blockIdx.y], last = offsets[blockIdx.y + 1];
        const long long i = (long long)first + (long long)blockIdx.x * 256 + (int)threadIdx.x; // (64 bits: first + the grid's width may pass 2^31)
        if (i >= last) return;
        double X, Y;
        const bool solved = undistorted_position(cams[blockIdx.y], uv[2 * (size_t)i], uv[2 * (size_t)i + 1], X, Y);
        xy[2 * (size_t)i] = X; xy[2 * (size_t)i + 1] = Y; // (two stores: the caller's array is 8-byte aligned only)
        if (ok) ok[i] = solved ? 1 : 0;
    }
    // The remap: four adjacent output pixels per lane, one word
    __global__ __launch_bounds__(256) void k_undistort_u8(const unsigned char *__restrict__ src, int Hs, int Ws, const float *__restrict__ map, int npx,
                                                          unsigned char *__restrict__ dst)
    {
        const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
        if (i0 >= npx) return;
        remap_four<1>({src}, Hs, Ws, map, {dst}, npx, i0);
    }
    // n images in one launch, the image index in blockIdx.y.  Image y's destination starts at byte y * npx of a caller's buffer,
    // so off a word boundary where npx is no multiple of 4: remap_four then stores byte by byte.
    __global__ __launch_bounds__(256) void k_undistort_u8_batch(const unsigned char *__restrict__ src, int Hs, int Ws, const float *__restrict__ map,
                                                                int npx, unsigned char *__restrict__ dst)
    {
        const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
        if (i0 >= npx) return;
        const size_t y = blockIdx.y;
        remap_four<1>({src + y * Hs * Ws}, Hs, Ws, map, {dst + y * npx}, npx, i0);
    }
    // The warp of n raw-geometry masks (include/mbavo.h: mbavo_undistort_mask_batch, mbavo_pairs_set_masks), mask y through map y:
    // the index in blockIdx.y, a lane four adjacent output bytes (camera_math.h: warp_mask_four).  Mask y's output starts at byte
    // y * dst_stride: npx for a caller's packed array (off a word where npx is no multiple of 4), the aligned stride of a pairs
    // batch's stored masks.
    __global__ __launch_bounds__(256) void k_undistort_mask_batch(const unsigned char *__restrict__ src, int Hs, int Ws, const float *__restrict__ maps,
                                                                  int npx, unsigned char *__restrict__ dst, long long dst_stride)
    {
        const int i0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
        if (i0 >= npx) return;
        const size_t y = blockIdx.y;
        warp_mask_four(src + y * Hs * Ws, Hs, Ws, maps + 2 * (size_t)npx * y, dst + y * (size_t)dst_stride, npx, i0);
    }

    // ---- the clearance mask of undistorted images (include/mbavo.h: mbavo_undistort_clearance_batch, mbavo_pairs_opts.valid_radius):
    // one byte per pixel of every pyramid level, 1 where no pixel within the radius has taken anything from outside the raw image.
    // Integer and comparison logic in three stages, each a function of the stage before alone: nothing is atomic, no workgroup
    // waits on another, and a byte does not depend on the grid or the alignment.  The map index is blockIdx.z / blockIdx.y.
    //
    // (a) "valid": levels 0 .. 3 from the map, a caller's mask or both (the two policies below) in one launch.  A workgroup takes a 64 x 16 tile of level 0, a lane four adjacent
    // pixels of a row (two 16-byte map loads, one word stored where the map and the destination allow it, else element by
    // element: a caller's packed pyramid, an odd H W); the tile stays in LDS and its 2 x 2 ANDs give the 32 x 8, 16 x 4 and 8 x 2
    // pixels of the next three levels -- the boxes of the 2 x 2 pyramid, which never straddle a tile.  Pixels of the tile
    // beyond the image are 0 and belong to no box of a level that exists.
    __device__ __forceinline__ unsigned and_2x2(const unsigned char (*s)[32], int lx, int ly)
    {
        return (unsigned)(s[2 * ly][2 * lx] & s[2 * ly][2 * lx + 1] & s[2 * ly + 1][2 * lx] & s[2 * ly + 1][2 * lx + 1]);
    }
    __device__ __forceinline__ void store_clear_pixel(unsigned char *__restrict__ out, const ClearLevels &lv, int l, int gx, int gy, unsigned v)
    {
        if (gx < lv.W[l] && gy < lv.H[l]) out[lv.off[l] + (size_t)gy * lv.W[l] + gx] = (unsigned char)v;
    }
    // The two terms of "valid at level 0" (include/mbavo.h), each a policy of k_clear_valid that is there or is not (an empty kernel
    // argument, no code).  The map term: map_entry_valid over the entries of map blockIdx.z.  The mask term: a byte != 0 of mask
    // blockIdx.z (H x W, undistorted geometry, `stride` bytes from one mask to the next), four bytes a lane, as one word where aligned.
    struct MapTerm
    {
        static constexpr bool present = true;
        const float *maps;
        int Hs, Ws;
    };
    struct NoMapTerm
    {
        static constexpr bool present = false;
    };
    struct MaskTerm
    {
        static constexpr bool present = true;
        const unsigned char *masks;
        long long stride;
        // pixels i .. i + 3 of the mask (the first `left` of them where the row ends): bit 8 j = pixel j usable
        __device__ __forceinline__ unsigned four(size_t mask, size_t i, bool whole, int left) const
        {
            const unsigned char *p = masks + mask * (size_t)stride + i;
            unsigned w = 0;
            if (whole && ((size_t)p & 3) == 0)
            {
                const unsigned v = *reinterpret_cast<const unsigned *>(p);
                w = ((v & 0xffu) ? 1u : 0u) | ((v & 0xff00u) ? 1u << 8 : 0u) | ((v & 0xff0000u) ? 1u << 16 : 0u) | ((v & 0xff000000u) ? 1u << 24 : 0u);
            }
            else
                for (int j = 0; j < 4 && j < left; ++j) w |= (unsigned)(p[j] != 0) << (8 * j);
            return w;
        }
    };
    struct NoMaskTerm
    {
        static constexpr bool present = false;
    };
    // (both in ONE kernel argument: a term that is not there takes no byte of it, and the map term alone is laid out as the three
    // arguments -- maps, Hs, Ws -- the kernel had before it took a mask)
    template <class MAP, class MASK>
    struct ValidTerms
    {
        [[no_unique_address]] MAP map;
        [[no_unique_address]] MASK mask;
    };
    template <class MAP, class MASK>
    __global__ __launch_bounds__(256) void k_clear_valid(const ValidTerms<MAP, MASK> vt, const ClearLevels lv, unsigned char *__restrict__ clear)
    {
        static_assert(MAP::present || MASK::present, "a valid stage without a term");
        const MASK &kt = vt.mask;
        __shared__ unsigned s0[16][16];           // level 0 of the tile, four pixels a word
        __shared__ unsigned char s1[8][32], s2[4][32]; // levels 1 and 2 (s2: 16 columns used)
        const int t = threadIdx.x, H = lv.H[0], W = lv.W[0];
        const float *__restrict__ map = nullptr;
        if constexpr (MAP::present) map = vt.map.maps + 2 * (size_t)H * W * blockIdx.z;
        unsigned char *__restrict__ out = clear + (size_t)lv.stride * blockIdx.z;
        const int x0 = (int)blockIdx.x * 64, y0 = (int)blockIdx.y * 16;
        {
            const int x = x0 + (t & 15) * 4, y = y0 + (t >> 4);
            unsigned word = 0;
            if (y < H && x < W)
            {
                const size_t i = (size_t)y * W + x;
                unsigned char *dst = out + lv.off[0] + i;
                const bool four = x + 4 <= W;
                if constexpr (MAP::present)
                {
                    const int Hs = vt.map.Hs, Ws = vt.map.Ws;
                    const float *m = map + 2 * i;
                    if (four && ((size_t)m & 15) == 0)
                    {
                        const float4 a = reinterpret_cast<const float4 *>(m)[0], b = reinterpret_cast<const float4 *>(m)[1];
                        word = (unsigned)map_entry_valid(a.x, a.y, Hs, Ws) | ((unsigned)map_entry_valid(a.z, a.w, Hs, Ws) << 8) |
                               ((unsigned)map_entry_valid(b.x, b.y, Hs, Ws) << 16) | ((unsigned)map_entry_valid(b.z, b.w, Hs, Ws) << 24);
                    }
                    else
                        for (int j = 0; j < 4 && x + j < W; ++j) word |= (unsigned)map_entry_valid(m[2 * j], m[2 * j + 1], Hs, Ws) << (8 * j);
                }
                else
                    word = four ? 0x01010101u : 0x01010101u >> (8 * (4 - (W - x))); // no map: every pixel of the image passes the map term
                if constexpr (MASK::present) word &= kt.four(blockIdx.z, i, four, W - x);
                if (four && ((size_t)dst & 3) == 0) *reinterpret_cast<unsigned *>(dst) = word;
                else
                    for (int j = 0; j < 4 && x + j < W; ++j) dst[j] = (unsigned char)((word >> (8 * j)) & 1u);
            }
            s0[t >> 4][t & 15] = word;
        }
        if (lv.L < 2) return; // (the same for the whole grid)
        __syncthreads();
        {
            const int lx = t & 31, ly = t >> 5, sh = (lx & 1) * 16; // pixels 2 lx, 2 lx + 1 of rows 2 ly, 2 ly + 1: half a word each
            const unsigned a = s0[2 * ly][lx >> 1] >> sh, b = s0[2 * ly + 1][lx >> 1] >> sh;
            const unsigned v = a & (a >> 8) & b & (b >> 8) & 1u;
            s1[ly][lx] = (unsigned char)v;
            store_clear_pixel(out, lv, 1, (x0 >> 1) + lx, (y0 >> 1) + ly, v);
        }
        if (lv.L < 3) return;
        __syncthreads();
        if (t < 64)
        {
            const int lx = t & 15, ly = t >> 4;
            const unsigned v = and_2x2(s1, lx, ly);
            s2[ly][lx] = (unsigned char)v;
            store_clear_pixel(out, lv, 2, (x0 >> 2) + lx, (y0 >> 2) + ly, v);
        }
        if (lv.L < 4) return;
        __syncthreads();
        if (t < 16) store_clear_pixel(out, lv, 3, (x0 >> 3) + (t & 7), (y0 >> 3) + (t >> 3), and_2x2(s2, t & 7, t >> 3));
    }
    // levels 4 .. L-1 in a second launch: a lane per pixel, the AND over its 2^(l-3) x 2^(l-3) pixels of level 3 (all of them
    // exist: (x + 1) 2^(l-3) <= (W >> l) 2^(l-3) <= W >> 3).  At most 1/256 of the level-0 pixels, at most 256 bytes a lane.
    __global__ __launch_bounds__(256) void k_clear_valid_coarse(const ClearLevels lv, unsigned char *__restrict__ clear)
    {
        const int blk = (int)blockIdx.x + lv.blk0[4];
        int l = 4;
        while (l + 1 < lv.L && blk >= lv.blk0[l + 1]) ++l;
        const int W = lv.W[l], W3 = lv.W[3], i = (blk - lv.blk0[l]) * 256 + (int)threadIdx.x;
        if (i >= lv.H[l] * W) return;
        unsigned char *__restrict__ out = clear + (size_t)lv.stride * blockIdx.y;
        const int y = i / W, x = i - y * W, s = 1 << (l - 3);
        const unsigned char *__restrict__ src = out + lv.off[3] + (size_t)(y * s) * W3 + x * s;
        unsigned v = 1;
        for (int j = 0; j < s; ++j)
            for (int k = 0; k < s; ++k) v &= src[(size_t)j * W3 + k];
        out[lv.off[l] + i] = (unsigned char)v;
    }
    // (b) "clear at radius r": the (2r + 1)^2 box AND as a row pass and a column pass over all levels (a level is walked as a
    // flat array of H*W pixels, its workgroups side by side in blockIdx.x).  A window that leaves the level is 0, so the result
    // carries a rectangular border of r.  Neighbouring lanes read neighbouring bytes; the 2r + 1 loads of a lane hit L1 / L2.
    template <bool COLUMNS>
    __global__ __launch_bounds__(256) void k_clear_box(const ClearLevels lv, int r, const unsigned char *__restrict__ src,
                                                       unsigned char *__restrict__ dst)
    {
        int l = 0;
        while (l + 1 < lv.L && (int)blockIdx.x >= lv.blk0[l + 1]) ++l;
        const int H = lv.H[l], W = lv.W[l], i = ((int)blockIdx.x - lv.blk0[l]) * 256 + (int)threadIdx.x;
        if (i >= H * W) return;
        const size_t base = (size_t)lv.stride * blockIdx.y + (size_t)lv.off[l];
        const unsigned char *__restrict__ s = src + base + i;
        const int y = i / W, x = i - y * W;
        const int at = COLUMNS ? y : x, n = COLUMNS ? H : W, step = COLUMNS ? W : 1;
        unsigned v = at >= r && at + r < n ? 1u : 0u;
        if (v)
            for (int d = -r; d <= r; ++d) v &= s[(long long)d * step]; // (at - r .. at + r: inside the row / the column)
        dst[base + i] = (unsigned char)v;
    }

    static bool image_size_valid(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W <= kUndistortMaxPixels; }

    static bool undistort_cams(int Hs, int Ws, const double from_intrinsics[4], const double dist[4], const double to_intrinsics[4], UndistortCams &m)
    {
        if (!to_intrinsics || !image_size_valid(Hs, Ws)) return false;
        if (from_intrinsics[0] == 0 || from_intrinsics[1] == 0 || to_intrinsics[0] == 0 || to_intrinsics[1] == 0) return false;
        m.to_fx = to_intrinsics[0]; m.to_fy = to_intrinsics[1]; m.to_cx = to_intrinsics[2]; m.to_cy = to_intrinsics[3];
        m.fx = from_intrinsics[0]; m.fy = from_intrinsics[1]; m.cx = from_intrinsics[2]; m.cy = from_intrinsics[3];
        m.k1 = dist[0]; m.k2 = dist[1]; m.p1 = dist[2]; m.p2 = dist[3];
        return true;
    }

    static bool undistort_cams(const mbavo_camera_radtan *from, const double to_intrinsics[4], UndistortCams &m)
    {
        if (!from) return false;
        return undistort_cams(from->H, from->W, from->intrinsics, from->dist, to_intrinsics, m);
    }

    static bool undistort_cams(const mbavo_camera_unified *from, const double to_intrinsics[4], UndistortCamsUnified &u)
    {
        if (!from || !(from->xi >= 0) || !std::isfinite(from->xi)) return false; // (a NaN fails the first comparison)
        u.xi = from->xi;
        return undistort_cams(from->H, from->W, from->intrinsics, from->dist, to_intrinsics, u.c);
    }

    template <class Camera, class Cams>
    static int undistort_map_of(Engine &eng, const Camera *from, const double to_intrinsics[4], int H, int W, float *d_map_xy)
    {
        Cams m;
        if (!d_map_xy || !image_size_valid(H, W) || !undistort_cams(from, to_intrinsics, m)) return MBAVO_E_ARG;
        const int npx = H * W;
        hipLaunchKernelGGL(k_undistort_map<Cams>, dim3((npx + 511) / 512), dim3(256), 0, eng.stream(), m, W, npx, d_map_xy);
        return (int)hipGetLastError();
    }

    int undistort_map(Engine &eng, const mbavo_camera_radtan *from, const double to_intrinsics[4], int H, int W, float *d_map_xy)
    {
        return undistort_map_of<mbavo_camera_radtan, UndistortCams>(eng, from, to_intrinsics, H, W, d_map_xy);
    }

    int undistort_map_unified(Engine &eng, const mbavo_camera_unified *from, const double to_intrinsics[4], int H, int W, float *d_map_xy)
    {
        return undistort_map_of<mbavo_camera_unified, UndistortCamsUnified>(eng, from, to_intrinsics, H, W, d_map_xy);
    }

    bool map_camera_of(const mbavo_pairs_camera &c, int H, int W, MapCamera &m)
    { // what undistort_map_of checks for the single call of the camera's model
        memset(&m, 0, sizeof(m));
        return image_size_valid(H, W) && map_camera_of(c, m);
    }

    bool map_camera_of(const mbavo_pairs_camera &c, MapCamera &m)
    { // the same without an H x W of the `to` image
        memset(&m, 0, sizeof(m));
        if (c.model == 1)
        {
            mbavo_camera_radtan from;
            from.H = c.H; from.W = c.W;
            memcpy(from.intrinsics, c.intrinsics, sizeof(from.intrinsics));
            memcpy(from.dist, c.dist, sizeof(from.dist));
            if (!undistort_cams(&from, c.to_intrinsics, m.u.c)) return false;
        }
        else if (c.model == 2)
        {
            mbavo_camera_unified from;
            from.H = c.H; from.W = c.W; from.xi = c.xi;
            memcpy(from.intrinsics, c.intrinsics, sizeof(from.intrinsics));
            memcpy(from.dist, c.dist, sizeof(from.dist));
            if (!undistort_cams(&from, c.to_intrinsics, m.u)) return false;
        }
        else
            return false;
        m.model = c.model;
        return true;
    }

    int undistort_map_batch_enqueue(Engine &eng, const MapCamera *d_cams, int n, int H, int W, float *d_maps)
    {
        const int npx = H * W;
        hipLaunchKernelGGL(k_undistort_map_batch, dim3((npx + 511) / 512, n), dim3(256), 0, eng.stream(), d_cams, W, npx, d_maps);
        return (int)hipGetLastError();
    }

    int undistort_map_batch(Engine &eng, int n, const mbavo_pairs_camera *h_cams, int H, int W, float *d_maps)
    {
        if (!h_cams || !d_maps || n < 1 || n > kUndistortMaxBatch || !image_size_valid(H, W)) return MBAVO_E_ARG;
        std::vector<MapCamera> cams((size_t)n);
        for (int i = 0; i < n; ++i)
            if (!map_camera_of(h_cams[i], H, W, cams[i])) return MBAVO_E_ARG;
        MapCamera *d_cams = (MapCamera *)eng.named_scratch(kMapCamerasSlot, sizeof(MapCamera) * cams.size());
        if (!d_cams) return (int)hipErrorOutOfMemory;
        // (a pageable source: the copy is staged before the call returns)
        const hipError_t e = hipMemcpyAsync(d_cams, cams.data(), sizeof(MapCamera) * cams.size(), hipMemcpyHostToDevice, eng.stream());
        if (e != hipSuccess) return (int)e;
        return undistort_map_batch_enqueue(eng, d_cams, n, H, W, d_maps);
    }

    int undistort_points_batch(Engine &eng, int n, const mbavo_pairs_camera *h_cams, const int *h_offsets, const double *d_uv, double *d_xy,
                               unsigned char *d_ok)
    {
        if (!h_cams || !h_offsets || n < 1 || n > kUndistortMaxBatch || h_offsets[0] != 0) return MBAVO_E_ARG;
        int longest = 0;
        for (int i = 0; i < n; ++i)
        {
            if (h_offsets[i + 1] < h_offsets[i]) return MBAVO_E_ARG;
            longest = std::max(longest, h_offsets[i + 1] - h_offsets[i]);
        }
        if (h_offsets[n] > 0 && (!d_uv || !d_xy)) return MBAVO_E_ARG;
        // [MapCamera n | offsets n + 1] in one copy
        const size_t cam_bytes = sizeof(MapCamera) * (size_t)n, bytes = cam_bytes + sizeof(int) * ((size_t)n + 1);
        std::vector<char> up(bytes);
        for (int i = 0; i < n; ++i)
            if (!map_camera_of(h_cams[i], reinterpret_cast<MapCamera *>(up.data())[i])) return MBAVO_E_ARG;
        memcpy(up.data() + cam_bytes, h_offsets, sizeof(int) * ((size_t)n + 1));
        if (longest == 0) return 0; // (no point: nothing to launch)
        char *dev = (char *)eng.named_scratch(kMapCamerasSlot, bytes);
        if (!dev) return (int)hipErrorOutOfMemory;
        // (a pageable source: the copy is staged before the call returns)
        const hipError_t e = hipMemcpyAsync(dev, up.data(), bytes, hipMemcpyHostToDevice, eng.stream());
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(k_undistort_points_batch, dim3((longest + 255) / 256, n), dim3(256), 0, eng.stream(), (const MapCamera *)dev,
                           (const int *)(dev + cam_bytes), d_uv, d_xy, d_ok);
        return (int)hipGetLastError();
    }

    int undistort_u8(Engine &eng, const unsigned char *d_src, int Hs, int Ws, const float *d_map_xy, int H, int W, unsigned char *d_dst)
    {
        if (!d_src || !d_map_xy || !d_dst || !image_size_valid(Hs, Ws) || !image_size_valid(H, W)) return MBAVO_E_ARG;
        const int npx = H * W;
        hipLaunchKernelGGL(k_undistort_u8, dim3((npx + 1023) / 1024), dim3(256), 0, eng.stream(), d_src, Hs, Ws, d_map_xy, npx, d_dst);
        return (int)hipGetLastError();
    }

    int undistort_u8_batch(Engine &eng, const unsigned char *d_src, int n, int Hs, int Ws, const float *d_map_xy, int H, int W, unsigned char *d_dst)
    {
        if (!d_src || !d_map_xy || !d_dst || n < 1 || n > kUndistortMaxBatch || !image_size_valid(Hs, Ws) || !image_size_valid(H, W)) return MBAVO_E_ARG;
        const int npx = H * W;
        hipLaunchKernelGGL(k_undistort_u8_batch, dim3((npx + 1023) / 1024, n), dim3(256), 0, eng.stream(), d_src, Hs, Ws, d_map_xy, npx, d_dst);
        return (int)hipGetLastError();
    }

    int clear_levels(int H, int W, int L, long long align, ClearLevels &lv)
    {
        memset(&lv, 0, sizeof(lv));
        if (L < 1 || L > 8 || !image_size_valid(H, W) || (H >> (L - 1)) < 1 || (W >> (L - 1)) < 1) return MBAVO_E_ARG;
        lv.L = L;
        for (int l = 0; l < L; ++l)
        {
            const long long px = (long long)(H >> l) * (W >> l);
            lv.H[l] = H >> l; lv.W[l] = W >> l;
            lv.off[l] = lv.stride;
            lv.stride += (px + align - 1) / align * align;
            lv.blk0[l + 1] = lv.blk0[l] + (int)((px + 255) / 256);
        }
        return 0;
    }

    int clearance_enqueue(Engine &eng, int n, const ClearSources &src, const ClearLevels &lv, int radius, unsigned char *d_clear, unsigned char *d_work)
    {
        hipStream_t st = eng.stream();
        const int L = lv.L;
        const dim3 grid((lv.W[0] + 63) / 64, (lv.H[0] + 15) / 16, n);
        const MapTerm mt{src.maps, src.Hs, src.Ws};
        const MaskTerm kt{src.masks, src.mask_stride};
        if (src.maps && src.masks)
            hipLaunchKernelGGL((k_clear_valid<MapTerm, MaskTerm>), grid, dim3(256), 0, st, ValidTerms<MapTerm, MaskTerm>{mt, kt}, lv, d_clear);
        else if (src.maps)
            hipLaunchKernelGGL((k_clear_valid<MapTerm, NoMaskTerm>), grid, dim3(256), 0, st, ValidTerms<MapTerm, NoMaskTerm>{mt, {}}, lv, d_clear);
        else
            hipLaunchKernelGGL((k_clear_valid<NoMapTerm, MaskTerm>), grid, dim3(256), 0, st, ValidTerms<NoMapTerm, MaskTerm>{{}, kt}, lv, d_clear);
        if (L > 4) hipLaunchKernelGGL(k_clear_valid_coarse, dim3(lv.blk0[L] - lv.blk0[4], n), dim3(256), 0, st, lv, d_clear);
        if (radius > 0)
        {
            hipLaunchKernelGGL(k_clear_box<false>, dim3(lv.blk0[L], n), dim3(256), 0, st, lv, radius, (const unsigned char *)d_clear, d_work);
            hipLaunchKernelGGL(k_clear_box<true>, dim3(lv.blk0[L], n), dim3(256), 0, st, lv, radius, (const unsigned char *)d_work, d_clear);
        }
        return (int)hipGetLastError();
    }

    int mask_clearance_batch(Engine &eng, int n, const float *d_maps, const unsigned char *d_masks, int H, int W, int Hs, int Ws, int L, int radius,
                             unsigned char *d_clear)
    {
        ClearLevels lv;
        if ((!d_maps && !d_masks) || !d_clear || n < 1 || n > kUndistortMaxBatch || radius < 0 || radius > kClearMaxRadius) return MBAVO_E_ARG;
        if (d_maps && !image_size_valid(Hs, Ws)) return MBAVO_E_ARG; // (no map: Hs, Ws are not read)
        if (clear_levels(H, W, L, 1, lv) != 0) return MBAVO_E_ARG;
        unsigned char *work = nullptr;
        if (radius > 0 && !(work = (unsigned char *)eng.named_scratch(kClearWorkSlot, (size_t)n * (size_t)lv.stride))) return (int)hipErrorOutOfMemory;
        return clearance_enqueue(eng, n, ClearSources{d_maps, d_maps ? Hs : 0, d_maps ? Ws : 0, d_masks, (long long)H * W}, lv, radius, d_clear, work);
    }

    int undistort_clearance_batch(Engine &eng, int n, const float *d_maps, int H, int W, int Hs, int Ws, int L, int radius, unsigned char *d_clear)
    {
        if (!d_maps) return MBAVO_E_ARG;
        return mask_clearance_batch(eng, n, d_maps, nullptr, H, W, Hs, Ws, L, radius, d_clear);
    }

    int undistort_mask_enqueue(Engine &eng, int n, const unsigned char *d_raw_masks, int Hs, int Ws, const float *d_maps, int H, int W,
                               unsigned char *d_masks, long long stride)
    {
        const int npx = H * W;
        hipLaunchKernelGGL(k_undistort_mask_batch, dim3((npx + 1023) / 1024, n), dim3(256), 0, eng.stream(), d_raw_masks, Hs, Ws, d_maps, npx, d_masks,
                           stride);
        return (int)hipGetLastError();
    }

    int undistort_mask_batch(Engine &eng, int n, const unsigned char *d_raw_masks, int Hs, int Ws, const float *d_maps, int H, int W,
                             unsigned char *d_masks)
    {
        if (!d_raw_masks || !d_maps || !d_masks || n < 1 || n > kUndistortMaxBatch || !image_size_valid(Hs, Ws) || !image_size_valid(H, W))
            return MBAVO_E_ARG;
        return undistort_mask_enqueue(eng, n, d_raw_masks, Hs, Ws, d_maps, H, W, d_masks, (long long)H * W);
    }

    int detect_cells_enqueue(Engine &eng, const unsigned char *d_img, int H, int W, int level, int im_H0, int im_W0, int cell_H,
                             int cell_W, float thr, CellPick *d_picks, int *num_cells)
    {
        if (!d_img || !d_picks || !num_cells || H < 1 || W < 1 || level < 0 || level > 30 || cell_H < 1 || cell_W < 1) return MBAVO_E_ARG;
        CellGrid g;
        const int rc = cell_grid(im_H0, im_W0, level, cell_H, cell_W, H, W, g);
        if (rc != 0) return rc;
        const int nc = g.cells_h * g.cells_w;
        hipLaunchKernelGGL(k_detect_cells, dim3(nc), dim3(64), 0, eng.stream(), d_img, H, W, g.ch, g.cw, g.cells_w, thr, (const float *)nullptr,
                           im_W0, std::pow(2, level), d_picks);
        *num_cells = nc;
        return (int)hipGetLastError();
    }
    int pyramid_enqueue(Engine &eng, unsigned char *const *d_levels, int H0, int W0, int L, hipStream_t on)
    { // levels 1 .. L-1 from level 0, three per launch (`on`: another stream than the engine's, or null)
        if (!d_levels || L < 1 || L > 8 || H0 < 1 || W0 < 1) return MBAVO_E_ARG;
        hipStream_t st_ = on ? on : eng.stream();
        for (int l = 0; l + 1 < L; l += 3)
        {
            const int n = L - 1 - l < 3 ? L - 1 - l : 3, Hs = H0 >> l, Ws = W0 >> l;
            if (Hs < 2 || Ws < 2) return MBAVO_E_ARG;
            hipLaunchKernelGGL(k_pyr_down_multi, dim3((Ws / 2 + 15) / 16, (Hs / 2 + 15) / 16), dim3(256), 0, st_, d_levels[l], Hs, Ws,
                               d_levels[l + 1], n >= 2 ? d_levels[l + 2] : nullptr, n >= 3 ? d_levels[l + 3] : nullptr, n);
        }
        return (int)hipGetLastError();
    }

    int keyframe_levels_enqueue(Engine &eng, unsigned char *const *d_levels, float *const *d_grads, int H0, int W0, int L, int cell_H, int cell_W,
                                float thr, CellPick *d_picks, int *cells_per_level, hipStream_t on)
    {
        if (!d_levels || !d_grads || L < 1 || L > 8) return MBAVO_E_ARG;
        hipStream_t st_ = on ? on : eng.stream();
        int rc = pyramid_enqueue(eng, d_levels, H0, W0, L, on);
        if (rc != 0) return rc;
        PyramidLevels lv;
        memset(&lv, 0, sizeof(lv));
        lv.n = L;
        const bool grid = d_picks != nullptr;
        for (int l = 0; l < L; ++l)
        {
            lv.img[l] = d_levels[l]; lv.grad[l] = (float2 *)d_grads[l];
            lv.H[l] = H0 >> l; lv.W[l] = W0 >> l;
            lv.row0[l + 1] = lv.row0[l] + lv.H[l];
            lv.scale[l] = std::pow(2, l);
            if (grid)
            {
                CellGrid g;
                if ((rc = cell_grid(H0, W0, l, cell_H, cell_W, lv.H[l], lv.W[l], g)) != 0) return rc;
                lv.ch[l] = g.ch; lv.cw[l] = g.cw; lv.cells_w[l] = g.cells_w;
                lv.cell0[l + 1] = lv.cell0[l] + g.cells_h * g.cells_w;
                if (cells_per_level) cells_per_level[l] = g.cells_h * g.cells_w;
            }
        }
        hipLaunchKernelGGL(k_gradients_multi, dim3((W0 + 255) / 256, lv.row0[L]), dim3(256), 0, st_, lv);
        if (grid) hipLaunchKernelGGL(k_detect_cells_multi, dim3(lv.cell0[L]), dim3(64), 0, st_, lv, thr, W0, d_picks);
        return (int)hipGetLastError();
    }
} // namespace mbavo

extern "C" int mbavo_gradient_magnitude_u8(const unsigned char *d_src, int H, int W, float *d_mag, void *stream)
{
    if (!d_src || !d_mag || H < 1 || W < 1) return MBAVO_E_ARG;
    hipLaunchKernelGGL(mbavo::k_grad_mag, dim3((W + 255) / 256, H), dim3(256), 0, (hipStream_t)stream, d_src, H, W, d_mag);
    return (int)hipGetLastError();
}

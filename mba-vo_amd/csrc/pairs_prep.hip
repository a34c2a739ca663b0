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
//   compaction                                                one workgroup per (pair, level): kept picks in row-major cell order
//
// The per-pixel detector functions are the per-image kernels' own (keyframe_math.h); the cell scan, the pyramid tile and the
// gradient arithmetic follow keyframe_ops.hip / image_ops.hip operation by operation: results are bit-identical to the per-image
// entry points (tests/test_gpu_pairs_prep.py holds every array to them).  The (pair, level) parameters live in a device-resident
// table written once at creation; a workgroup finds its entry from the grid index.  All streaming work, HBM-bound.
#include "pairs_prep.h"
#include "keyframe_math.h"
#include "pixel_math.h"
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
        CellPick *picks;          // `cells` of them
        int H, W, ch, cw, cells_w, cells, border;
        double scale;             // 2^level
    };
    // where the levels start in the grids that run over all levels of a pair (by value: L <= 8)
    struct PairsGrid
    {
        int L, B;
        int blk0[9];  // gradients: first workgroup of every level
        int cell0[9]; // grid selection: first cell of every level
    };

    namespace pairs
    {
        constexpr long long kAlign = 256;
        // largest level-0 image: one row of the strided level-0 copy is a whole image (tested at this size)
        constexpr long long kMaxPixels = 1ll << 22;
        inline long long align_up(long long v, long long a) { return (v + a - 1) / a * a; }

        // ---- pyramids: k_pyr_down_multi (keyframe_ops.hip) over 2B images; image z < B is pair z's keyframe, else pair (z - B)'s
        // current frame; levels l0 + 1 .. l0 + n below level l0
        __global__ __launch_bounds__(256) void k_pairs_pyr_down(const PairLevelDesc *__restrict__ desc, int B, int L, int l0, int n)
        {
            __shared__ int t1[16][17], t2[8][9];
            const int tid = threadIdx.x, z = blockIdx.z;
            const PairLevelDesc *d = desc + (size_t)(z < B ? z : z - B) * L + l0;
            const bool key = z < B;
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
        __global__ __launch_bounds__(256) void k_pairs_gradients(const PairLevelDesc *__restrict__ desc, const PairsGrid g)
        {
            constexpr int PPL = GradOut<FORMAT>::kPixels;
            int l = 0;
            while (l + 1 < g.L && (int)blockIdx.x >= g.blk0[l + 1]) ++l;
            const PairLevelDesc &d = desc[(size_t)blockIdx.y * g.L + l];
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

        // ---- grid selection: detect_cell of keyframe_ops.hip (same per-pixel functions, keyframe_math.h) with the border test
        // one wave per cell, four cells per workgroup; grid (ceil(cells of a pair / 4), B)
        __global__ __launch_bounds__(256) void k_pairs_detect(const PairLevelDesc *__restrict__ desc, const PairsGrid g, float thr,
                                                              const float *__restrict__ depth_all, int H0, int W0)
        {
            const int lane = threadIdx.x & 63, cell = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
            if (cell >= g.cell0[g.L]) return; // (whole waves)
            int l = 0;
            while (l + 1 < g.L && cell >= g.cell0[l + 1]) ++l;
            const PairLevelDesc &d = desc[(size_t)blockIdx.y * g.L + l];
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
                    const float *depth = depth_all + (size_t)blockIdx.y * H0 * W0; // the pair's own map
                    const int m = d.border;
                    const bool inside = p.x >= m && p.x < W - m && p.y >= m && p.y < H - m;
                    p.keep = (depth_of(depth, W0, d.scale, p.x, p.y, p.z) && inside) ? 1 : 0;
                }
                d.picks[ci] = p;
            }
        }

        // ---- ordered compaction: one workgroup per (pair, level), grid (L, B).  256 cells per step: every wave ballots its 64
        // cells, the four wave totals meet in LDS, a kept pick's place is (kept so far) + (earlier waves) + (earlier lanes).
        __global__ __launch_bounds__(256) void k_pairs_compact(const PairLevelDesc *__restrict__ desc, int *__restrict__ counts)
        {
            __shared__ int wave_total[4];
            const int e = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
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
    } // namespace pairs

    using namespace pairs;

    int pairs_plan(const mbavo_pairs_opts *o, PairsPlan &p)
    {
        if (!o) return MBAVO_E_ARG;
        memset(&p, 0, sizeof(p));
        const int B = o->B, L = o->L;
        if (B < 1 || B > 32767 || L < 1 || L > 8 || o->H < 1 || o->W < 1) return MBAVO_E_ARG;
        if ((o->H >> (L - 1)) < 8 || (o->W >> (L - 1)) < 8 || (long long)o->H * o->W > kMaxPixels) return MBAVO_E_ARG;
        if ((o->spline_deg_k != 2 && o->spline_deg_k != 4) || o->N < o->spline_deg_k || o->N > 16) return MBAVO_E_ARG;
        if (o->cell_H < 1 || o->cell_W < 1 || o->keyframe_format < 0 || o->keyframe_format > 2) return MBAVO_E_ARG;
        p.B = B; p.L = L; p.N = o->N; p.format = o->keyframe_format; p.grad_bytes = o->keyframe_format == 0 ? 8 : 4;
        for (int l = 0; l < L; ++l)
        {
            if (o->S[l] < 1 || o->P[l] < 1 || !o->pattern_xy[l] || o->border[l] < 0) return MBAVO_E_ARG;
            const int Hl = o->H >> l, Wl = o->W >> l;
            // FeatureDetectorBase.cpp:56-64 (as detect_semidense, keyframe_ops.hip)
            const int sf = (int)std::pow(2, l);
            const int ch = (int)(o->cell_H / std::pow(1.414, l)), cw = (int)(o->cell_W / std::pow(1.414, l));
            if (ch < 1 || cw < 1) return MBAVO_E_ARG; // the reference divides by zero here
            const int cells_h = (o->H / sf) / ch + 1, cells_w = (o->W / sf) / cw + 1;
            // (level l is (H >> l) x (W >> l) = the size the grid is made for: every pixel's cell exists, so detect_semidense's
            // MBAVO_E_RANGE -- an image larger than the grid of the H0 x W0 it is given -- cannot occur here)
            p.H[l] = Hl; p.W[l] = Wl; p.ch[l] = ch; p.cw[l] = cw; p.cells_w[l] = cells_w; p.cells[l] = cells_h * cells_w;
            p.cell0[l + 1] = p.cell0[l] + p.cells[l];
            p.px0[l + 1] = p.px0[l] + align_up((long long)Hl * Wl, 16);
            p.kp0[l + 1] = p.kp0[l] + 3ll * align_up(p.cells[l], 2);
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
        p.off_picks = take((long long)B * p.cell0[L] * (long long)sizeof(CellPick));
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
        if (!arena_ && !h_counts_ && !h_motion_) return;
        (void)hipSetDevice(eng_.device());
        (void)hipStreamSynchronize(eng_.stream());
        if (arena_) (void)hipFree(arena_);
        if (h_counts_) (void)hipHostFree(h_counts_);
        if (h_motion_) (void)hipHostFree(h_motion_);
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
        if ((e = hipMalloc((void **)&arena_, (size_t)p.total)) != hipSuccess) { arena_ = nullptr; return (int)e; }
        if ((e = hipHostMalloc((void **)&h_counts_, sizeof(int) * B * L)) != hipSuccess) { h_counts_ = nullptr; return (int)e; }
        if ((e = hipHostMalloc((void **)&h_motion_, sizeof(double) * B * (2 + 7 * N))) != hipSuccess) { h_motion_ = nullptr; return (int)e; }
        hipStream_t st = eng_.stream();
        // deterministic contents for what a prepare does not write (pads) and for the motion before set_motion
        if ((e = hipMemsetAsync(arena_, 0, (size_t)p.total, st)) != hipSuccess) return (int)e;

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
                d.kp_z = d.kp_xy + 2 * align_up(p.cells[l], 2);
                d.picks = (CellPick *)(arena_ + p.off_picks) + (long long)b * p.cell0[L] + p.cell0[l];
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

    int PairBatch::prepare(const unsigned char *d_sharp, const float *d_depth_z, const unsigned char *d_blur, int *h_counts)
    {
        if (!arena_ || !d_sharp || !d_depth_z || !d_blur) return MBAVO_E_ARG;
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
        PairsGrid g;
        memset(&g, 0, sizeof(g));
        g.L = L; g.B = B;
        const int ppl = p.format == 0 ? 2 : 4;
        for (int l = 0; l < L; ++l)
        {
            g.blk0[l + 1] = g.blk0[l] + (p.H[l] * p.W[l] + 256 * ppl - 1) / (256 * ppl);
            g.cell0[l + 1] = p.cell0[l + 1];
        }
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
        hipLaunchKernelGGL(k_pairs_detect, dim3((p.cell0[L] + 3) / 4, B), dim3(256), 0, st, desc, g, opts_.score_threshold, d_depth_z, p.H[0], p.W[0]);
        hipLaunchKernelGGL(k_pairs_compact, dim3(L, B), dim3(256), 0, st, desc, d_counts);
        stats_[0] += 3;
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        if ((e = hipMemcpyAsync(h_counts_, d_counts, sizeof(int) * B * L, hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
        stats_[2] = (long long)sizeof(int) * B * L;
        e = hipStreamSynchronize(st);
        stats_[1] = 1;
        if (e != hipSuccess) return (int)e;
        for (int i = 0; i < B * L; ++i) probs_[i].K = h_counts_[i];
        if (h_counts) memcpy(h_counts, h_counts_, sizeof(int) * B * L);
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
        if ((e = hipMemcpyAsync(arena_ + plan_.off_motion, m, sizeof(double) * B * (2 + 7 * N), hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return (int)e; // (the staging buffer is free again)
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

    void PairBatch::last_stats(long long out[4]) const
    {
        out[0] = stats_[0]; out[1] = stats_[1]; out[2] = stats_[2];
        out[3] = arena_ ? plan_.total : 0;
    }
} // namespace mbavo

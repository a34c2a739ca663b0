// pairs_photo.hip -- each pair's brightness gain and offset against its keyframe (include/mbavo.h: mbavo_pairs_match_brightness):
// I_cur = a I_key + b fitted on the aligned patches of one level by iteratively reweighted least squares under the Huber weight,
// and optionally removed from the pair's current-frame pyramid inside the object.  ONE launch per round on the refinement's grid
// and one more for the cost under the final (a, b); with apply one launch over the level-0 frames and the pyramid launches of
// prepare and update.
//
// The evaluation -- prologue, the intensity-only item, the tiles -- is pairs_depth_eval.h's depth_photo; what is this kernel's own
// is its policy, PhotoStep:
//
//   begin        the round's (a, b): (1, 0) in round 0, else what the round before left on the device; a pair an earlier round
//                found degenerate has nothing to do
//   item         the fit residual under (a, b), its squared Huber weight and cost
//   keypoint     the six sums over a full keypoint's P items in the evaluation's order, added to the lane's
//   record       seven sums, closed as the refinement closes its four (close_record); the lane that closes them solves the 2 x 2
//                normal equations, judges the pair and hands (a, b) to the next round
#include "pairs_depth_eval.h"

namespace mbavo
{
    namespace pairs
    {
        // ww s, (ww s) s, (ww s) c, ww c of a keypoint's items as patch_rho_sum reads its terms
        struct PhotoWx
        {
            const double *ww, *x;
            __host__ __device__ double operator[](int i) const
            {
#pragma clang fp contract(off)
                return ww[i] * x[i];
            }
        };
        struct PhotoWxy
        {
            const double *ww, *x, *y;
            __host__ __device__ double operator[](int i) const
            {
#pragma clang fp contract(off)
                return (ww[i] * x[i]) * y[i];
            }
        };

        struct PhotoStep
        {
            const PhotoArgs &a;
            mbavo_pairs_photo_opts o;
            double ga = 1.0, gb = 0.0;
            double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; // n, Sx, Sy, Sxx, Sxy, C
            int n_full = 0;

            __device__ __forceinline__ explicit PhotoStep(const PhotoArgs &args) : a(args) {}

            __device__ __forceinline__ void off_knots(const DepthEvalSlot &c)
            {
                if (threadIdx.x == 0 && c.grp == 0)
                {
                    struct mbavo_pairs_photo *out = a.out + c.b;
                    const double nan = __builtin_nan("");
                    out->status = MBAVO_E_RANGE; out->num_keypoints = c.K; out->num_full = 0; out->num_pixels = 0;
                    out->gain = nan; out->offset = nan; out->cost_before = nan; out->cost_after = nan;
                }
            }

            // (the record and (a, b) of a pair are written by the lane that takes the pair's LAST ticket of a launch, behind every
            // read of them here)
            __device__ __forceinline__ bool begin(const DepthEvalSlot &c)
            {
                o = *a.opts;
                if (a.round == 0) return true;
                if (a.out[c.b].status != 0) return false;
                ga = a.ab[2 * c.b]; gb = a.ab[2 * c.b + 1];
                return true;
            }

            __device__ __forceinline__ void item(const DepthEvalSlot &, double s, double cur, double &ww, double &rho) const
            {
#pragma clang fp contract(off)
                const double e = cur - (ga * s + gb);
                double w;
                huber_weight(e, o.huber, w, rho);
                ww = w * w;
            }

            __device__ __forceinline__ void keypoint(const DepthEvalSlot &c, int, bool full, const PhotoPatch &p)
            {
#pragma clang fp contract(off)
                if (!full) return;
                ++n_full;
                sum[0] = sum[0] + patch_rho_sum(p.u0, c.P);
                sum[1] = sum[1] + patch_rho_sum(PhotoWx{p.u0, p.s}, c.P);
                sum[2] = sum[2] + patch_rho_sum(PhotoWx{p.u0, p.c}, c.P);
                sum[3] = sum[3] + patch_rho_sum(PhotoWxy{p.u0, p.s, p.s}, c.P);
                sum[4] = sum[4] + patch_rho_sum(PhotoWxy{p.u0, p.s, p.c}, c.P);
                sum[5] = sum[5] + patch_rho_sum(p.u1, c.P);
            }

            __device__ __forceinline__ void finish(const DepthEvalSlot &c, double *s_w)
            {
                const double mine[kPhotoSums] = {sum[0], sum[1], sum[2], sum[3], sum[4], sum[5], (double)n_full}; // (an integer below 2^53: exact)
                double r[kPhotoSums];
                if (!close_record<kPhotoSums>(mine, s_w, a.ev.partials, a.ev.tickets, c.ent, c.grp, c.G, r)) return;
                struct mbavo_pairs_photo *out = a.out + c.b;
                const int R = o.rounds;
                if (a.round == R)
                { // the launch behind the last round: the cost under the final (a, b)
                    out->cost_after = r[5];
                    return;
                }
                const int n_pix = (int)r[6] * c.P;
                if (a.round == 0)
                {
                    out->status = 0; out->num_keypoints = c.K; out->num_full = (int)r[6]; out->num_pixels = n_pix;
                    out->cost_before = r[5];
                }
                bool degenerate;
                double ga1, gb1;
                {
#pragma clang fp contract(off)
                    const double n = r[0], Sx = r[1], Sy = r[2], Sxx = r[3], Sxy = r[4];
                    const double det = n * Sxx - Sx * Sx;
                    ga1 = (n * Sxy - Sx * Sy) / det;
                    gb1 = (Sy - ga1 * Sx) / n;
                    degenerate = n_pix < o.min_pixels || !(det > (o.min_var * n) * n) || !__builtin_isfinite(ga1) || !__builtin_isfinite(gb1) ||
                                 ga1 < o.gain_min || ga1 > o.gain_max;
                }
                if (degenerate)
                {
                    out->status = MBAVO_PHOTO_DEGENERATE;
                    out->gain = 1.0; out->offset = 0.0;
                    out->cost_after = a.round == 0 ? r[5] : out->cost_before;
                    return;
                }
                out->gain = ga1; out->offset = gb1;
                a.ab[2 * c.b] = ga1; a.ab[2 * c.b + 1] = gb1;
            }
        };

        template <int KDEG>
        __global__ __launch_bounds__(256) void k_pairs_photo_fit(const PhotoArgs a)
        {
            extern __shared__ double s_dyn[]; // [S pose entries | the prologue's segments]
            __shared__ DepthPhotoLds sh;
            PhotoStep step(a);
            depth_photo<KDEG>(a.ev, sh, s_dyn, step);
        }

        // ---- the correction: v -> min(255, max(0, rint((v - b) / a))) on the level-0 current frame of every pair with status 0.
        // A grey level has 256 values: lane v of a workgroup forms the image of v once, and the pixels look theirs up in LDS, 16 per
        // lane (level 0 of an image starts on a 256-byte boundary).  Workgroup (x, b) serves pixels [4096 x, 4096 (x + 1)) of pair b.
        __global__ __launch_bounds__(256) void k_pairs_photo_apply(const PairLevelDesc *__restrict__ desc, const struct mbavo_pairs_photo *__restrict__ rec,
                                                                   int L)
        {
            __shared__ unsigned char lut[256];
            const int b = (int)blockIdx.y, tid = (int)threadIdx.x;
            if (rec[b].status != 0) return; // (the same in every lane)
            {
#pragma clang fp contract(off)
                const double ga = rec[b].gain, gb = rec[b].offset;
                double v = __builtin_rint(((double)tid - gb) / ga);
                v = v > 0.0 ? v : 0.0;
                v = v < 255.0 ? v : 255.0;
                lut[tid] = (unsigned char)v;
            }
            __syncthreads();
            const PairLevelDesc &d = desc[(size_t)b * L];
            const int npx = d.H * d.W, i0 = ((int)blockIdx.x * 256 + tid) * 16;
            if (i0 >= npx) return;
            unsigned char *img = d.cur + i0;
            if (i0 + 16 <= npx)
            {
                uint4 q = *reinterpret_cast<const uint4 *>(img);
                unsigned char px[16];
                __builtin_memcpy(px, &q, 16);
#pragma unroll
                for (int j = 0; j < 16; ++j) px[j] = lut[px[j]];
                __builtin_memcpy(&q, px, 16);
                *reinterpret_cast<uint4 *>(img) = q;
            }
            else
                for (int j = 0; i0 + j < npx; ++j) img[j] = lut[img[j]];
        }
    } // namespace pairs

    using namespace pairs;

    // (follows refine_depths where the two agree: the checks, the call, the dispatch)
    int PairBatch::match_brightness(const mbavo_pairs_photo_opts *o, struct mbavo_pairs_photo *h_out)
    {
        DepthCall &call = photo_call_;
        call.stats = CallStats{};
        if (!arena_ || !prepared_ || !motion_set_ || !o) return MBAVO_E_ARG;
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L, k = opts_.spline_deg_k;
        if (o->level < 0 || o->level >= L || o->rounds < 0 || o->rounds > 8 || !flags01({o->apply}) || o->min_pixels < 0) return MBAVO_E_ARG;
        if (bad_limit(o->huber) || bad_limit(o->min_var) || bad_limit(o->gain_min) || bad_limit(o->gain_max)) return MBAVO_E_ARG;
        mbavo_pairs_photo_opts opt = *o;
        if (opt.rounds == 0) opt.rounds = 3;
        if (opt.min_pixels == 0) opt.min_pixels = 64;
        if (opt.huber == 0.0) opt.huber = opts_.huber_a;
        if (opt.min_var == 0.0) opt.min_var = 4.0;
        if (opt.gain_min == 0.0) opt.gain_min = 0.25;
        if (opt.gain_max == 0.0) opt.gain_max = 4.0;
        if (opt.gain_min > opt.gain_max) return MBAVO_E_ARG;
        PhotoArgs a{};
        int width;
        size_t lds;
        if (depth_eval_args(o->level, a.ev, width, lds) != 0) return MBAVO_E_ARG;
        if (lds + sizeof(DepthPhotoLds) + 512 > 160 * 1024) return MBAVO_E_ARG; // (the kernel's static LDS: 34 080 B)
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        const size_t rec = sizeof(struct mbavo_pairs_photo) * (size_t)B;
        if ((e = call.open(rec, kPhotoSums, PhotoScratch::opt_bytes(B), 1)) != hipSuccess) return (int)e;
        *(mbavo_pairs_photo_opts *)call.h_opts = opt;
        if ((e = call.upload(sizeof(mbavo_pairs_photo_opts))) != hipSuccess) return (int)e;
        const PhotoScratch scratch{call};
        a.opts = scratch.opts(); a.ab = scratch.ab(); a.out = scratch.records();
        a.ev.partials = call.partials; a.ev.tickets = call.tickets;
        const int rc = dispatch<2, 4>(k, [&](auto kd) { // (no gradient taps: the keyframe's format makes no difference to the kernel)
            auto kernel = k_pairs_photo_fit<decltype(kd)::value>;
            const hipError_t le = eng_.ensure_lds((const void *)kernel, lds);
            if (le != hipSuccess) return (int)le;
            for (a.round = 0; a.round <= opt.rounds; ++a.round)
            {
                hipLaunchKernelGGL(kernel, dim3(width, B), dim3(256), lds, st, a);
                ++call.stats.launches;
            }
            return 0;
        });
        if (rc != 0) return rc;
        if (opt.apply == 1)
        {
            hipLaunchKernelGGL(k_pairs_photo_apply, dim3((p.H[0] * p.W[0] + 4095) / 4096, B), dim3(256), 0, st, lay_.desc(arena_), scratch.records(), L);
            ++call.stats.launches;
            pyramids(0, nullptr, B, call.stats);
        }
        return call.finish(h_out, rec);
    }
} // namespace mbavo

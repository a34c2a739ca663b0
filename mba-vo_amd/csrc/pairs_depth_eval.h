// pairs_depth_eval.h -- what the aligned blurred frame says about one keypoint's depth, ONCE for the kernels that use it
// (pairs_refine.hip: k_pairs_refine, the damped step; pairs_filter.hip: k_pairs_filter, the recursive inverse-depth filter;
// pairs_search.hip: k_pairs_search, the exhaustive search over candidate depths, through depth_search below; pairs_photo.hip:
// k_pairs_photo_fit, each pair's brightness gain and offset, through depth_photo below):
// include/mbavo.h, mbavo_pairs_refine_depths steps 1 - 6 and 9.  A kernel is depth_eval<KDEG, GRAD>(args, LDS, step) with `step`
// its policy, as the keypoint kernels take their camera:
//
//   step.off_knots(c)                      every lane of a workgroup whose pair has a sample off its knots (nothing evaluated)
//   step.begin(c)                          every lane, once the pose entries are in LDS
//   step.keypoint(c, kp, nv, full, g, h, cost)   the lane of keypoint kp of the tile: valid pixels, and for a full keypoint the
//                                          gradient, curvature and cost of step 6 (zeros otherwise); lanes add their own sums
//   step.finish(c, s_w)                    every lane: the record (close_record)
//
//   prologue     the S pose entries of the pair at this level's sample times into LDS (pose_entries.h, the fused kernels' own
//                prologue without the Jacobian columns); a sample off the knots ends the workgroup in step.off_knots
//   items        the level's keypoints in tiles of T = min(256, 1024 / P); a lane per (keypoint, pixel): the patch centre at the
//                mid-exposure entry (reference order), the truncated pixel, the S warps with the taps of two samples in flight
//                (pixel_math.h: sample_issue, tap_blend), residual, its depth derivative, Huber
//   keypoints    a lane per keypoint of the tile: the P-segment sums in the evaluation's order (patch_rho_sum), then the policy
//
// The evaluation's bodies are called, not restated; the one thing formed here is the derivative of a sample's tap coordinates
// with respect to the plane depth (depth_terms).  No floating-point atomics: the one integer ticket per (pair, level) decides WHICH
// workgroup adds the partials, never the order in which they are added, so the same bits come back from run to run and for any B.
#ifndef MBAVO_PAIRS_DEPTH_EVAL_H
#define MBAVO_PAIRS_DEPTH_EVAL_H

#include "pairs_prep.h"
#include "pairs_desc.h"
#include "pose_entries.h"
#include "pixel_math.h"
#include <cmath>
#include <hip/hip_runtime.h>

namespace mbavo
{
    namespace pairs
    {
        // the static LDS of a depth kernel: three doubles and a byte per item, the waves' sums (25 bytes per item)
        struct DepthEvalLds
        {
            double rho[kRefineItems], g[kRefineItems], h[kRefineItems], w[4];
            unsigned char ok[kRefineItems];
        };

        // the (pair, level) a workgroup serves and its share of it
        struct DepthEvalSlot
        {
            int ent, b, l, K, P, grp, G, T; // ent: the record; grp of G workgroups; T: keypoints of a tile
            long long o0;                   // the level's first entry in the caller's per-keypoint arrays
            double *kp_z;
        };

        // the workgroup's sums in a fixed order -- butterfly within the wave, then the four waves in wave order -- in every lane
        __device__ __forceinline__ double refine_block_sum(double v, double *s_w)
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
            __syncthreads(); // (the last sum has been read)
            if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
            __syncthreads();
            return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
        }

        // ONE lane per workgroup, r its workgroup's NV sums: with G > 1 they go to parts[grp] and the lane that takes the LAST
        // ticket of the (pair, level) gets in r the G partials added from 0.0 in the order g = 0 .. G-1; true in the lane that
        // writes the record (the hand-over of engine.hip's ticket_finalize: agent-scope release, ticket, acquire by the last one)
        template <int NV>
        __device__ __forceinline__ bool group_sums(double (&r)[NV], double *parts, int *ticket, int grp, int G)
        {
            if (G == 1) return true;
            double *mine = parts + NV * grp;
            for (int j = 0; j < NV; ++j) mine[j] = r[j];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            if (atomicAdd(ticket, 1) != G - 1) return false;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            {
#pragma clang fp contract(off)
                for (int j = 0; j < NV; ++j) r[j] = 0.0;
                for (int g = 0; g < G; ++g)
                    for (int j = 0; j < NV; ++j) r[j] = r[j] + __hip_atomic_load(parts + NV * g + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // ready for the next call
            return true;
        }

        // the close of a record: every lane hands in its NV sums `mine`; they are summed over the workgroup one after the other in
        // array order (refine_block_sum), then over the G workgroups of entry `ent` (group_sums).  True in the ONE lane that writes
        // the record, with the sums in r
        template <int NV>
        __device__ __forceinline__ bool close_record(const double (&mine)[NV], double *s_w, double *partials, int *tickets, int ent, int grp, int G,
                                                     double (&r)[NV])
        {
#pragma unroll
            for (int j = 0; j < NV; ++j) r[j] = refine_block_sum(mine[j], s_w);
            if (threadIdx.x != 0) return false;
            return group_sums<NV>(r, partials + (size_t)ent * kRefineGroups * NV, tickets + ent, grp, G);
        }

        // (gx du + gy dv) of one sample: du, dv = the derivative of its tap coordinates with respect to the plane depth at the
        // fixed pixel -- u = fx Px iz + cx with Px = (D - t_z) C1 r_x + t_x and iz = 1 / (D + 1e-8)
        template <int KDEG>
        __device__ __forceinline__ double depth_terms(const PoseEntry<KDEG> &pe, const SampleInFlight &f, double iz, const Camera &cam, double gx,
                                                      double gy)
        {
#pragma clang fp contract(off)
            const double Px = f.sc * f.rx + pe.t[0];
            const double Py = f.sc * f.ry + pe.t[1];
            const double du = cam.fx * (((f.C1 * f.rx) * iz) - ((Px * iz) * iz));
            const double dv = cam.fy * (((f.C1 * f.ry) * iz) - ((Py * iz) * iz));
            return gx * du + gy * dv;
        }

        template <int KDEG, int GRAD, class Step>
        __device__ __forceinline__ void depth_eval(const DepthEvalArgs &a, DepthEvalLds &sh, double *s_dyn, Step &step)
        {
            double *s_rho = sh.rho, *s_g = sh.g, *s_h = sh.h;
            unsigned char *s_ok = sh.ok;
            const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
            const int ent = (int)blockIdx.y, grp = (int)blockIdx.x;
            const int b = ent / a.levels, li = ent - b * a.levels, l = a.level < 0 ? li : a.level;
            const size_t e = (size_t)b * a.L + l;
            const int S = a.S[l], P = a.P[l], K = a.counts[e];
            const int G = a.groups[l];
            if (grp >= G) return; // (the grid's width is the widest level's)
            PoseEntry<KDEG> *tab = (PoseEntry<KDEG> *)s_dyn;
            SplineSeg *segs = (SplineSeg *)(tab + S);
            const PairLevelDesc &pd = a.desc[e];
            DepthEvalSlot c;
            c.ent = ent; c.b = b; c.l = l; c.K = K; c.P = P; c.grp = grp; c.G = G;
            c.T = kRefineItems / P < 256 ? kRefineItems / P : 256;
            c.o0 = (long long)b * a.out_stride + a.out0[l];
            c.kp_z = pd.kp_z;

            // ---- the pose entries, and whether every sample time lies on the knots
            ProblemDesc d{};
            d.cap = a.cap + b; d.exp_t = a.exp + b;
            d.t0 = a.t0[b]; d.dt = a.dt; d.S = S; d.N = a.N;
            const double *kt = a.kt + (size_t)b * 3 * a.N, *kR = a.kR + (size_t)b * 4 * a.N;
            int off = 0;
            for (int s = tid; s < S; s += 256)
            {
                int idx;
                double u;
                bool oob;
                pose_sample_segment<KDEG>(d, 0, s, idx, u, oob);
                const double ts = d.cap[0] - d.exp_t[0] * 0.5 + s * d.exp_t[0] / (S - 1 + 1e-8);
                if (oob || !(ts == ts)) off = 1;
            }
            if (__syncthreads_or(off))
            {
                step.off_knots(c);
                return;
            }
            frame_pose_entries<KDEG, false>(d, kt, kR, 0, tab, segs, wave, lane, nullptr, false);
            __syncthreads();

            Camera cam;
            {
                const double sc = (double)(1 << l);
                const double *k0 = a.of_pair ? &a.of_pair[b].fx : a.intr;
                cam.fx = k0[0] / sc; cam.fy = k0[1] / sc; cam.cx = k0[2] / sc; cam.cy = k0[3] / sc;
                cam.H = pd.H; cam.W = pd.W;
            }
            const unsigned char *I_ref = pd.ref, *I_cur = pd.cur;
            const float *G_ref = (const float *)pd.grad;
            const double *kp_xy = pd.kp_xy;
            double *kp_z = pd.kp_z;
            const int *pat = a.pattern + a.pat0[l];
            const PoseEntry<KDEG> &mid = tab[S / 2]; // patch centres use sample S / 2, as the evaluation
            const double mid_rt[3] = {mid.rt[0], mid.rt[1], mid.rt[2]}, mid_q[4] = {mid.q[0], mid.q[1], mid.q[2], mid.q[3]};
            const double fS = (double)(float)S, inv_S = 1.0 / fS;
            const int T = c.T;
            step.begin(c);

            for (int tile = grp * T; tile < K; tile += G * T)
            {
                const int nk = K - tile < T ? K - tile : T, items = nk * P;
                for (int it = tid; it < items; it += 256)
                {
                    const int kpl = it / P, j = it - kpl * P, kp = tile + kpl;
                    const double kx = kp_xy[2 * (size_t)kp], ky = kp_xy[2 * (size_t)kp + 1], D = kp_z[kp];
                    double ox, oy;
                    patch_centre_rt(mid_rt, mid_q, kx, ky, D, cam, ox, oy);
                    const int px = (int)(ox + pat[2 * j]); // truncation, as pixel_row_sum
                    const int py = (int)(oy + pat[2 * j + 1]);
                    bool ok = !(px < 0 || px > cam.W - 1 || py < 0 || py > cam.H - 1);
                    double res = 0.0, dd = 0.0;
                    if (ok)
                    {
                        const double cur = (double)((const MBAVO_GLOBAL unsigned char *)I_cur)[py * cam.W + px];
                        double ray[3];
                        unit_ray(cam, (double)px, (double)py, ray);
                        const double iz = reciprocal(D + 1e-8);
                        double isum = 0.0, acc = 0.0;
                        // two samples' taps in flight, retired in sample order (pixel_row_sum's pairs, its remainder for odd S)
                        SampleInFlight fa, fb;
                        auto retire = [&](const PoseEntry<KDEG> &pe, const SampleInFlight &f, bool first) {
#pragma clang fp contract(off)
                            double val, gx = 0, gy = 0;
                            tap_blend<true, GRAD>(f.taps, val, gx, gy);
                            isum = first ? val : isum + val;
                            acc = acc + depth_terms<KDEG>(pe, f, iz, cam, gx, gy);
                            ok = ok && f.taps.ok;
                        };
                        int s = 0;
                        for (; s + 1 < S; s += 2)
                        {
                            sample_issue<KDEG, true, GRAD>(tab[s], ray, D, iz, cam, I_ref, G_ref, fa);
                            sample_issue<KDEG, true, GRAD>(tab[s + 1], ray, D, iz, cam, I_ref, G_ref, fb);
                            retire(tab[s], fa, s == 0);
                            retire(tab[s + 1], fb, false);
                        }
                        if (s < S)
                        {
                            sample_issue<KDEG, true, GRAD>(tab[s], ray, D, iz, cam, I_ref, G_ref, fa);
                            retire(tab[s], fa, s == 0);
                        }
                        if (ok)
                        {
#pragma clang fp contract(off)
                            res = quotient(isum, fS) - cur;
                            dd = inv_S * acc;
                        }
                    }
                    double w, rho;
                    huber_weight(res, a.huber_a, w, rho);
                    {
#pragma clang fp contract(off)
                        const double ww = w * w;
                        s_rho[it] = rho;
                        s_g[it] = ok ? (ww * res) * dd : 0.0;
                        s_h[it] = ok ? (ww * dd) * dd : 0.0;
                        s_ok[it] = ok ? 1 : 0;
                    }
                }
                __syncthreads();
                if (tid < nk)
                { // (T <= 256: a lane has at most one keypoint of a tile)
#pragma clang fp contract(off)
                    int nv = 0;
                    for (int j = 0; j < P; ++j) nv += s_ok[tid * P + j];
                    const bool full = nv == P;
                    double g = 0.0, h = 0.0, cst = 0.0;
                    if (full)
                    {
                        cst = patch_rho_sum((const double *)(s_rho + tid * P), P);
                        g = patch_rho_sum((const double *)(s_g + tid * P), P);
                        h = patch_rho_sum((const double *)(s_h + tid * P), P);
                    }
                    step.keypoint(c, tile + tid, nv, full, g, h, cst);
                }
                __syncthreads(); // (the tile's LDS is free again; the depths of the next tile are other keypoints')
            }
            step.finish(c, sh.w);
        }

        // ---- the exhaustive counterpart (pairs_search.hip: k_pairs_search; include/mbavo.h, mbavo_pairs_search_depths): the patch
        // cost alone -- steps 1 - 6 without the gradient taps -- at ND candidate depths per keypoint, the patch centre moving with
        // the candidate.  A kernel is depth_search<KDEG>(args, LDS, step) on depth_eval's grid and tiles, `step` its policy:
        //
        //   step.off_knots(c), step.begin(c), step.finish(c, s_w)     as depth_eval's
        //   step.candidates()                      ND, the same in every lane
        //   step.range(D, lo, st)                  the first candidate's inverse depth and the spacing of a keypoint at depth D
        //   step.candidate(c, kp, d, cost)         the lane of keypoint kp, d ascending from 0: the cost of candidate d, NaN if one
        //                                          of its P pixels is invalid
        //   step.keypoint(c, kp)                   the same lane, once all ND candidates have been handed over
        //
        // kSearchBatch candidates are evaluated between two barriers: a lane per (keypoint, pixel) writes their rho_j to LDS, a
        // lane per keypoint sums them.
        constexpr int kSearchBatch = 4;
        struct DepthSearchLds
        {
            double rho[kSearchBatch][kRefineItems], w[4]; // (NaN: the pixel is invalid at that candidate)
        };

        // rho_j of one pixel (pattern offset dx, dy) of the keypoint (kx, ky) at depth D, NaN if the pixel is invalid: depth_eval's
        // item without the derivative
        template <int KDEG>
        __device__ __forceinline__ double depth_item_rho(const PoseEntry<KDEG> *tab, int S, const double (&mid_rt)[3], const double (&mid_q)[4],
                                                         const Camera &cam, const unsigned char *I_ref, const float *G_ref, const unsigned char *I_cur,
                                                         double kx, double ky, double D, int dx, int dy, double fS, double huber_a)
        {
            double ox, oy;
            patch_centre_rt(mid_rt, mid_q, kx, ky, D, cam, ox, oy);
            const int px = (int)(ox + dx); // truncation, as pixel_row_sum
            const int py = (int)(oy + dy);
            bool ok = !(px < 0 || px > cam.W - 1 || py < 0 || py > cam.H - 1);
            double res = 0.0;
            if (ok)
            {
                const double cur = (double)((const MBAVO_GLOBAL unsigned char *)I_cur)[py * cam.W + px];
                double ray[3];
                unit_ray(cam, (double)px, (double)py, ray);
                const double iz = reciprocal(D + 1e-8);
                double isum = 0.0;
                SampleInFlight fa, fb;
                auto retire = [&](const SampleInFlight &f, bool first) {
#pragma clang fp contract(off)
                    double val, gx = 0, gy = 0;
                    tap_blend<false>(f.taps, val, gx, gy);
                    isum = first ? val : isum + val;
                    ok = ok && f.taps.ok;
                };
                int s = 0;
                for (; s + 1 < S; s += 2)
                {
                    sample_issue<KDEG, false>(tab[s], ray, D, iz, cam, I_ref, G_ref, fa);
                    sample_issue<KDEG, false>(tab[s + 1], ray, D, iz, cam, I_ref, G_ref, fb);
                    retire(fa, s == 0);
                    retire(fb, false);
                }
                if (s < S)
                {
                    sample_issue<KDEG, false>(tab[s], ray, D, iz, cam, I_ref, G_ref, fa);
                    retire(fa, s == 0);
                }
                if (ok)
                {
#pragma clang fp contract(off)
                    res = quotient(isum, fS) - cur;
                }
            }
            double w, rho;
            huber_weight(res, huber_a, w, rho);
            return ok ? rho : __builtin_nan("");
        }

        template <int KDEG, class Step>
        __device__ __forceinline__ void depth_search(const DepthEvalArgs &a, DepthSearchLds &sh, double *s_dyn, Step &step)
        {
            const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
            const int ent = (int)blockIdx.y, grp = (int)blockIdx.x;
            const int b = ent / a.levels, li = ent - b * a.levels, l = a.level < 0 ? li : a.level;
            const size_t e = (size_t)b * a.L + l;
            const int S = a.S[l], P = a.P[l], K = a.counts[e];
            const int G = a.groups[l];
            if (grp >= G) return; // (the grid's width is the widest level's)
            PoseEntry<KDEG> *tab = (PoseEntry<KDEG> *)s_dyn;
            SplineSeg *segs = (SplineSeg *)(tab + S);
            const PairLevelDesc &pd = a.desc[e];
            DepthEvalSlot c;
            c.ent = ent; c.b = b; c.l = l; c.K = K; c.P = P; c.grp = grp; c.G = G;
            c.T = kRefineItems / P < 256 ? kRefineItems / P : 256;
            c.o0 = (long long)b * a.out_stride + a.out0[l];
            c.kp_z = pd.kp_z;

            // ---- the pose entries, and whether every sample time lies on the knots (depth_eval's prologue)
            ProblemDesc d{};
            d.cap = a.cap + b; d.exp_t = a.exp + b;
            d.t0 = a.t0[b]; d.dt = a.dt; d.S = S; d.N = a.N;
            const double *kt = a.kt + (size_t)b * 3 * a.N, *kR = a.kR + (size_t)b * 4 * a.N;
            int off = 0;
            for (int s = tid; s < S; s += 256)
            {
                int idx;
                double u;
                bool oob;
                pose_sample_segment<KDEG>(d, 0, s, idx, u, oob);
                const double ts = d.cap[0] - d.exp_t[0] * 0.5 + s * d.exp_t[0] / (S - 1 + 1e-8);
                if (oob || !(ts == ts)) off = 1;
            }
            if (__syncthreads_or(off))
            {
                step.off_knots(c);
                return;
            }
            frame_pose_entries<KDEG, false>(d, kt, kR, 0, tab, segs, wave, lane, nullptr, false);
            __syncthreads();

            Camera cam;
            {
                const double sc = (double)(1 << l);
                const double *k0 = a.of_pair ? &a.of_pair[b].fx : a.intr;
                cam.fx = k0[0] / sc; cam.fy = k0[1] / sc; cam.cx = k0[2] / sc; cam.cy = k0[3] / sc;
                cam.H = pd.H; cam.W = pd.W;
            }
            const unsigned char *I_ref = pd.ref, *I_cur = pd.cur;
            const float *G_ref = (const float *)pd.grad;
            const double *kp_xy = pd.kp_xy;
            const double *kp_z = pd.kp_z;
            const int *pat = a.pattern + a.pat0[l];
            const PoseEntry<KDEG> &mid = tab[S / 2]; // patch centres use sample S / 2, as the evaluation
            const double mid_rt[3] = {mid.rt[0], mid.rt[1], mid.rt[2]}, mid_q[4] = {mid.q[0], mid.q[1], mid.q[2], mid.q[3]};
            const double fS = (double)(float)S;
            const int T = c.T;
            step.begin(c);
            const int ND = step.candidates();

            for (int tile = grp * T; tile < K; tile += G * T)
            {
                const int nk = K - tile < T ? K - tile : T, items = nk * P;
                for (int d0 = 0; d0 < ND; d0 += kSearchBatch)
                {
                    const int nb = ND - d0 < kSearchBatch ? ND - d0 : kSearchBatch;
                    for (int it = tid; it < items; it += 256)
                    {
                        const int kpl = it / P, j = it - kpl * P, kp = tile + kpl;
                        const double kx = kp_xy[2 * (size_t)kp], ky = kp_xy[2 * (size_t)kp + 1];
                        const int dx = pat[2 * j], dy = pat[2 * j + 1];
                        double lo, st;
                        step.range(kp_z[kp], lo, st);
                        for (int i = 0; i < nb; ++i)
                        {
                            double D;
                            {
#pragma clang fp contract(off)
                                D = 1.0 / (lo + (double)(d0 + i) * st);
                            }
                            sh.rho[i][it] = depth_item_rho<KDEG>(tab, S, mid_rt, mid_q, cam, I_ref, G_ref, I_cur, kx, ky, D, dx, dy, fS, a.huber_a);
                        }
                    }
                    __syncthreads();
                    if (tid < nk) // (T <= 256: a lane has at most one keypoint of a tile)
                        for (int i = 0; i < nb; ++i) step.candidate(c, tile + tid, d0 + i, patch_rho_sum((const double *)(sh.rho[i] + tid * P), P));
                    __syncthreads(); // (the batch's LDS is free again)
                }
                if (tid < nk) step.keypoint(c, tile + tid); // (the depths a store here changes are read by no other lane from here on)
            }
            step.finish(c, sh.w);
        }

        // ---- the photometric counterpart (pairs_photo.hip: k_pairs_photo_fit; include/mbavo.h, mbavo_pairs_match_brightness): per
        // item what the keyframe predicts and what the current frame shows -- depth_item_sc at the keypoint's own depth -- on
        // depth_eval's grid and tiles.  A kernel is depth_photo<KDEG>(args, LDS, step), `step` its policy:
        //
        //   step.off_knots(c), step.finish(c, s_w)     as depth_eval's
        //   step.begin(c)                          every lane, once the pose entries are in LDS; false (in every lane of the
        //                                          workgroup alike): the pair has nothing to do, nothing is handed in
        //   step.item(c, s, cur, u0, u1)           the lane of a VALID item: two numbers of the policy's own kept beside s and c
        //   step.keypoint(c, kp, full, patch)      the lane of keypoint kp of the tile: whether all P pixels are valid and, for a
        //                                          full keypoint, its P items (PhotoPatch); lanes add their own sums
        struct DepthPhotoLds
        {
            double s[kRefineItems], c[kRefineItems], u0[kRefineItems], u1[kRefineItems], w[4];
            unsigned char ok[kRefineItems];
        };
        struct PhotoPatch
        {
            const double *s, *c, *u0, *u1; // P entries each
        };

        // what one pixel (pattern offset dx, dy) of the keypoint (kx, ky) at depth D sees -- depth_item_rho's item before the residual
        // is formed (the same calls in the same order; that function stays as it is so that the search kernel's code does): the
        // synthesised keyframe intensity syn = quotient(sum_s I_s, fS) and the current frame's grey level cur, both 0.0 where the
        // pixel is invalid; true: the pixel is valid
        template <int KDEG>
        __device__ __forceinline__ bool depth_item_sc(const PoseEntry<KDEG> *tab, int S, const double (&mid_rt)[3], const double (&mid_q)[4],
                                                      const Camera &cam, const unsigned char *I_ref, const float *G_ref, const unsigned char *I_cur,
                                                      double kx, double ky, double D, int dx, int dy, double fS, double &syn, double &cur)
        {
            double ox, oy;
            patch_centre_rt(mid_rt, mid_q, kx, ky, D, cam, ox, oy);
            const int px = (int)(ox + dx); // truncation, as pixel_row_sum
            const int py = (int)(oy + dy);
            bool ok = !(px < 0 || px > cam.W - 1 || py < 0 || py > cam.H - 1);
            syn = 0.0; cur = 0.0;
            if (ok)
            {
                const double c = (double)((const MBAVO_GLOBAL unsigned char *)I_cur)[py * cam.W + px];
                double ray[3];
                unit_ray(cam, (double)px, (double)py, ray);
                const double iz = reciprocal(D + 1e-8);
                double isum = 0.0;
                SampleInFlight fa, fb;
                auto retire = [&](const SampleInFlight &f, bool first) {
#pragma clang fp contract(off)
                    double val, gx = 0, gy = 0;
                    tap_blend<false>(f.taps, val, gx, gy);
                    isum = first ? val : isum + val;
                    ok = ok && f.taps.ok;
                };
                int s = 0;
                for (; s + 1 < S; s += 2)
                {
                    sample_issue<KDEG, false>(tab[s], ray, D, iz, cam, I_ref, G_ref, fa);
                    sample_issue<KDEG, false>(tab[s + 1], ray, D, iz, cam, I_ref, G_ref, fb);
                    retire(fa, s == 0);
                    retire(fb, false);
                }
                if (s < S)
                {
                    sample_issue<KDEG, false>(tab[s], ray, D, iz, cam, I_ref, G_ref, fa);
                    retire(fa, s == 0);
                }
                if (ok)
                {
                    syn = quotient(isum, fS);
                    cur = c;
                }
            }
            return ok;
        }

        template <int KDEG, class Step>
        __device__ __forceinline__ void depth_photo(const DepthEvalArgs &a, DepthPhotoLds &sh, double *s_dyn, Step &step)
        {
            const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
            const int ent = (int)blockIdx.y, grp = (int)blockIdx.x;
            const int b = ent / a.levels, li = ent - b * a.levels, l = a.level < 0 ? li : a.level;
            const size_t e = (size_t)b * a.L + l;
            const int S = a.S[l], P = a.P[l], K = a.counts[e];
            const int G = a.groups[l];
            if (grp >= G) return; // (the grid's width is the widest level's)
            PoseEntry<KDEG> *tab = (PoseEntry<KDEG> *)s_dyn;
            SplineSeg *segs = (SplineSeg *)(tab + S);
            const PairLevelDesc &pd = a.desc[e];
            DepthEvalSlot c;
            c.ent = ent; c.b = b; c.l = l; c.K = K; c.P = P; c.grp = grp; c.G = G;
            c.T = kRefineItems / P < 256 ? kRefineItems / P : 256;
            c.o0 = (long long)b * a.out_stride + a.out0[l];
            c.kp_z = pd.kp_z;

            // ---- the pose entries, and whether every sample time lies on the knots (depth_eval's prologue)
            ProblemDesc d{};
            d.cap = a.cap + b; d.exp_t = a.exp + b;
            d.t0 = a.t0[b]; d.dt = a.dt; d.S = S; d.N = a.N;
            const double *kt = a.kt + (size_t)b * 3 * a.N, *kR = a.kR + (size_t)b * 4 * a.N;
            int off = 0;
            for (int s = tid; s < S; s += 256)
            {
                int idx;
                double u;
                bool oob;
                pose_sample_segment<KDEG>(d, 0, s, idx, u, oob);
                const double ts = d.cap[0] - d.exp_t[0] * 0.5 + s * d.exp_t[0] / (S - 1 + 1e-8);
                if (oob || !(ts == ts)) off = 1;
            }
            if (__syncthreads_or(off))
            {
                step.off_knots(c);
                return;
            }
            frame_pose_entries<KDEG, false>(d, kt, kR, 0, tab, segs, wave, lane, nullptr, false);
            __syncthreads();

            Camera cam;
            {
                const double sc = (double)(1 << l);
                const double *k0 = a.of_pair ? &a.of_pair[b].fx : a.intr;
                cam.fx = k0[0] / sc; cam.fy = k0[1] / sc; cam.cx = k0[2] / sc; cam.cy = k0[3] / sc;
                cam.H = pd.H; cam.W = pd.W;
            }
            const unsigned char *I_ref = pd.ref, *I_cur = pd.cur;
            const float *G_ref = (const float *)pd.grad;
            const double *kp_xy = pd.kp_xy;
            const double *kp_z = pd.kp_z;
            const int *pat = a.pattern + a.pat0[l];
            const PoseEntry<KDEG> &mid = tab[S / 2]; // patch centres use sample S / 2, as the evaluation
            const double mid_rt[3] = {mid.rt[0], mid.rt[1], mid.rt[2]}, mid_q[4] = {mid.q[0], mid.q[1], mid.q[2], mid.q[3]};
            const double fS = (double)(float)S;
            const int T = c.T;
            if (!step.begin(c)) return;

            for (int tile = grp * T; tile < K; tile += G * T)
            {
                const int nk = K - tile < T ? K - tile : T, items = nk * P;
                for (int it = tid; it < items; it += 256)
                {
                    const int kpl = it / P, j = it - kpl * P, kp = tile + kpl;
                    double syn, cur, u0 = 0.0, u1 = 0.0;
                    const bool ok = depth_item_sc<KDEG>(tab, S, mid_rt, mid_q, cam, I_ref, G_ref, I_cur, kp_xy[2 * (size_t)kp], kp_xy[2 * (size_t)kp + 1],
                                                        kp_z[kp], pat[2 * j], pat[2 * j + 1], fS, syn, cur);
                    if (ok) step.item(c, syn, cur, u0, u1);
                    sh.s[it] = syn; sh.c[it] = cur; sh.u0[it] = u0; sh.u1[it] = u1;
                    sh.ok[it] = ok ? 1 : 0;
                }
                __syncthreads();
                if (tid < nk)
                { // (T <= 256: a lane has at most one keypoint of a tile)
                    int nv = 0;
                    for (int j = 0; j < P; ++j) nv += sh.ok[tid * P + j];
                    const int o = tid * P;
                    step.keypoint(c, tile + tid, nv == P, PhotoPatch{sh.s + o, sh.c + o, sh.u0 + o, sh.u1 + o});
                }
                __syncthreads(); // (the tile's LDS is free again)
            }
            step.finish(c, sh.w);
        }

        template <int KDEG>
        static size_t refine_lds(int S)
        {
            return sizeof(PoseEntry<KDEG>) * (size_t)S + sizeof(SplineSeg) * (size_t)(kPoseSPB * (KDEG - 1));
        }

        // the options refinement and filter share (both structs name them alike): MBAVO_E_ARG by the header's rules, else 0 and
        // in `opt` the options with the defaults for 0 filled in
        template <class Opts>
        static int depth_step_opts(const Opts *o, int L, Opts &opt)
        {
            if (o->level < -1 || o->level >= L || !flags01({o->apply})) return MBAVO_E_ARG;
            if (bad_limit(o->min_info) || bad_limit(o->max_rel_step) || o->max_rel_step >= 1.0) return MBAVO_E_ARG;
            opt = *o;
            if (opt.max_rel_step == 0.0) opt.max_rel_step = 0.25;
            return depth_limits(opt.z_min, opt.z_max);
        }
    } // namespace pairs
} // namespace mbavo

#endif

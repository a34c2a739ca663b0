// pairs_refine.hip -- what the aligned blurred frame says about every keypoint's depth (include/mbavo.h: mbavo_pairs_refine_depths):
// per keypoint the gradient and Gauss-Newton curvature of its blur-aware patch cost with respect to its plane depth, the
// trajectory held at its estimate, and the damped inverse-depth step, optionally written in place.  ONE launch; a reported (pair,
// level) is served by G = min(kRefineGroups, ceil(capacity / T)) workgroups, workgroup g taking the tiles g, g + G, g + 2 G, .. of its
// keypoints (the grid is sized by the capacity, never by a count read back; a workgroup without a tile only hands in zeros):
//
//   prologue     the S pose entries of the pair at this level's sample times into LDS (pose_entries.h, the fused kernels' own
//                prologue without the Jacobian columns); a sample off the knots ends the workgroup with an MBAVO_E_RANGE record
//   items        the level's keypoints in tiles of T = min(256, 1024 / P); a lane per (keypoint, pixel): the patch centre at the
//                mid-exposure entry (reference order), the truncated pixel, the S warps with the taps of two samples in flight
//                (pixel_math.h: sample_issue, tap_blend), residual, its depth derivative, Huber
//   keypoints    a lane per keypoint of the tile: the P-segment sums in the evaluation's order (patch_rho_sum), the step, the
//                optional store of the new depth, the lane's share of the record sums
//   record       butterfly within each wave, the four waves in order: the workgroup's four partial sums into scratch; the workgroup
//                that takes the LAST ticket of its (pair, level) adds the G partials in the order g = 0 .. G-1 and writes the record
//
// The evaluation's bodies are called, not restated; the one thing formed here is the derivative of a sample's tap coordinates
// with respect to the plane depth (depth_terms).  No floating-point atomics: the one integer ticket per (pair, level) decides WHICH
// workgroup adds the partials, never the order in which they are added, so the same bits come back from run to run and for any B.
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

        template <int KDEG, int GRAD>
        __global__ __launch_bounds__(256) void k_pairs_refine(const RefineArgs a)
        {
            extern __shared__ double s_dyn[]; // [S pose entries | the prologue's segments]
            __shared__ double s_rho[kRefineItems], s_g[kRefineItems], s_h[kRefineItems], s_w[4];
            __shared__ unsigned char s_ok[kRefineItems];
            const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
            const int ent = (int)blockIdx.y, grp = (int)blockIdx.x;
            const int b = ent / a.levels, li = ent - b * a.levels, l = a.level < 0 ? li : a.level;
            const size_t e = (size_t)b * a.L + l;
            const int S = a.S[l], P = a.P[l], K = a.counts[e];
            struct mbavo_pairs_refine *out = a.out + ent;
            const int G = a.groups[l];
            if (grp >= G) return; // (the grid's width is the widest level's)
            PoseEntry<KDEG> *tab = (PoseEntry<KDEG> *)s_dyn;
            SplineSeg *segs = (SplineSeg *)(tab + S);

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
                if (tid == 0 && grp == 0)
                {
                    const double nan = __builtin_nan("");
                    out->status = MBAVO_E_RANGE; out->num_keypoints = K; out->num_full = 0; out->num_moved = 0;
                    out->cost = nan; out->sum_sq_rel = nan;
                }
                return;
            }
            frame_pose_entries<KDEG, false>(d, kt, kR, 0, tab, segs, wave, lane, nullptr, false);
            __syncthreads();

            const PairLevelDesc &pd = a.desc[e];
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
            const mbavo_pairs_refine_opts o = *a.opts;
            const long long o0 = (long long)b * a.out_stride + a.out0[l];
            const int T = kRefineItems / P < 256 ? kRefineItems / P : 256;

            double cost_sum = 0.0, rel_sum = 0.0;
            int n_full = 0, n_moved = 0;
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
                    const int kp = tile + tid;
                    int nv = 0;
                    for (int j = 0; j < P; ++j) nv += s_ok[tid * P + j];
                    const bool full = nv == P;
                    double g = 0.0, h = 0.0, c = 0.0;
                    if (full)
                    {
                        c = patch_rho_sum((const double *)(s_rho + tid * P), P);
                        g = patch_rho_sum((const double *)(s_g + tid * P), P);
                        h = patch_rho_sum((const double *)(s_h + tid * P), P);
                    }
                    if (a.g) a.g[o0 + kp] = g;
                    if (a.h) a.h[o0 + kp] = h;
                    if (a.cost) a.cost[o0 + kp] = c;
                    if (a.valid) a.valid[o0 + kp] = nv;
                    if (full)
                    {
                        ++n_full;
                        cost_sum = cost_sum + c;
                        const double D = kp_z[kp];
                        const double rho = 1.0 / D, DD = D * D;
                        const double g_rho = -(DD * g), h_rho = (DD * DD) * h;
                        if (h_rho > o.min_info && h_rho > 0.0)
                        {
                            const double m = o.max_rel_step * rho;
                            double d_rho = -g_rho / h_rho;
                            if (d_rho > m) d_rho = m;
                            if (d_rho < -m) d_rho = -m;
                            const double D_new = 1.0 / (rho + d_rho);
                            if (__builtin_isfinite(D_new) && D_new >= o.z_min && (o.z_max == 0.0 || D_new <= o.z_max))
                            {
                                const double rel = d_rho / rho;
                                ++n_moved;
                                rel_sum = rel_sum + rel * rel;
                                if (o.apply == 1) kp_z[kp] = D_new;
                            }
                        }
                    }
                }
                __syncthreads(); // (the tile's LDS is free again; the depths of the next tile are other keypoints')
            }
            // ---- the record: this workgroup's partial sums, then the last workgroup of the (pair, level) adds all G in group order
            const double cost = refine_block_sum(cost_sum, s_w), ssr = refine_block_sum(rel_sum, s_w);
            const double nf = refine_block_sum((double)n_full, s_w), nm = refine_block_sum((double)n_moved, s_w); // (integers below 2^53: exact)
            if (tid != 0) return;
            double *parts = a.partials + (size_t)ent * kRefineGroups * 4;
            if (G > 1)
            { // (the hand-over of engine.hip's ticket_finalize: agent-scope release, ticket, acquire by the last one)
                double *mine = parts + 4 * grp;
                mine[0] = cost; mine[1] = ssr; mine[2] = nf; mine[3] = nm;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                if (atomicAdd(&a.tickets[ent], 1) != G - 1) return;
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            }
            double r[4] = {cost, ssr, nf, nm};
            if (G > 1)
            {
#pragma clang fp contract(off)
                for (int j = 0; j < 4; ++j) r[j] = 0.0;
                for (int g = 0; g < G; ++g)
                    for (int j = 0; j < 4; ++j) r[j] = r[j] + __hip_atomic_load(parts + 4 * g + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&a.tickets[ent], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // ready for the next call
            }
            out->status = 0; out->num_keypoints = K; out->num_full = (int)r[2]; out->num_moved = (int)r[3];
            out->cost = r[0]; out->sum_sq_rel = r[1];
        }

        template <int KDEG>
        static size_t refine_lds(int S)
        {
            return sizeof(PoseEntry<KDEG>) * (size_t)S + sizeof(SplineSeg) * (size_t)(kPoseSPB * (KDEG - 1));
        }
    } // namespace pairs

    using namespace pairs;

    int PairBatch::refine_depths(const mbavo_pairs_refine_opts *o, struct mbavo_pairs_refine *h_out, double *d_g, double *d_h, double *d_cost,
                                 int *d_valid)
    {
        ref_stats_ = CallStats{};
        if (!arena_ || !prepared_ || !motion_set_ || !o) return MBAVO_E_ARG;
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L, k = opts_.spline_deg_k;
        if (o->level < -1 || o->level >= L || (o->apply != 0 && o->apply != 1)) return MBAVO_E_ARG;
        for (double v : {o->min_info, o->max_rel_step, o->z_min, o->z_max})
            if (!std::isfinite(v) || v < 0.0) return MBAVO_E_ARG;
        if (o->max_rel_step >= 1.0) return MBAVO_E_ARG;
        mbavo_pairs_refine_opts opt = *o;
        if (opt.max_rel_step == 0.0) opt.max_rel_step = 0.25;
        if (opt.z_min == 0.0) opt.z_min = 1e-2;
        if (opt.z_max != 0.0 && opt.z_max < opt.z_min) return MBAVO_E_ARG;
        const int levels = o->level < 0 ? L : 1;
        size_t lds = 0;
        for (int i = 0; i < levels; ++i)
        {
            const int l = o->level < 0 ? i : o->level;
            if (opts_.P[l] > kRefineItems) return MBAVO_E_ARG;
            const size_t need = k == 2 ? refine_lds<2>(opts_.S[l]) : refine_lds<4>(opts_.S[l]);
            lds = need > lds ? need : lds;
        }
        // (the static arrays: three doubles and a byte per item, the waves' sums)
        if (lds + (size_t)kRefineItems * 25 + 64 > 160 * 1024) return MBAVO_E_ARG;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        const size_t rec_bytes = sizeof(struct mbavo_pairs_refine) * (size_t)B * levels, opt_bytes = sizeof(mbavo_pairs_refine_opts);
        const size_t rec_bytes_max = sizeof(struct mbavo_pairs_refine) * (size_t)B * L;
        const long long o_parts = align_up((long long)sizeof(struct mbavo_pairs_refine) * B * L, kAlign);
        const long long o_tickets = o_parts + align_up((long long)sizeof(double) * 4 * kRefineGroups * B * L, kAlign);
        const long long o_opts = o_tickets + align_up((long long)sizeof(int) * B * L, kAlign);
        // the first call: its scratch (include/mbavo.h)
        if (!refine_)
        { // (the tickets start at zero; the last workgroup of a (pair, level) leaves its ticket at zero again)
            if ((e = refine_.alloc((size_t)o_opts + opt_bytes)) != hipSuccess) return (int)e;
            if ((e = hipMemsetAsync(refine_ + o_tickets, 0, sizeof(int) * (size_t)B * L, st)) != hipSuccess) return (int)e;
        }
        if (!h_refine_ && (e = h_refine_.alloc(rec_bytes_max + opt_bytes)) != hipSuccess) return (int)e;
        if (!opts_copied_)
        {
            e = hipEventCreateWithFlags(&opts_copied_, hipEventDisableTiming);
            if (e != hipSuccess)
            {
                opts_copied_ = nullptr;
                return (int)e;
            }
        }
        else
        { // (an earlier call that waited for nothing may still be reading the options' mirror)
            if ((e = hipEventSynchronize(opts_copied_)) != hipSuccess) return (int)e;
        }
        mbavo_pairs_refine_opts *h_opts = (mbavo_pairs_refine_opts *)(h_refine_ + rec_bytes_max);
        *h_opts = opt;
        const mbavo_pairs_refine_opts *d_opts = (const mbavo_pairs_refine_opts *)(refine_ + o_opts);
        if ((e = hipMemcpyAsync((void *)d_opts, h_opts, opt_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        if ((e = hipEventRecord(opts_copied_, st)) != hipSuccess) return (int)e;
        RefineArgs a{};
        a.desc = lay_.desc(arena_); a.counts = lay_.counts(arena_); a.pattern = lay_.pattern(arena_);
        a.cap = lay_.cap(arena_); a.exp = lay_.exp(arena_); a.t0 = lay_.t0(arena_);
        a.kt = lay_.knots_t(arena_); a.kR = lay_.knots_R(arena_);
        a.of_pair = opts_.num_cameras > 0 ? lay_.pair_cameras(arena_) : nullptr;
        a.opts = d_opts;
        for (int i = 0; i < 4; ++i) a.intr[i] = opts_.intrinsics[i];
        a.dt = probs_[0].dt; a.huber_a = opts_.huber_a;
        a.L = L; a.N = p.N; a.level = o->level; a.levels = levels;
        long long at = 0;
        int width = 1;
        for (int l = 0; l < L; ++l)
        {
            a.S[l] = opts_.S[l]; a.P[l] = opts_.P[l]; a.pat0[l] = p.pat0[l];
            const int T = kRefineItems / a.P[l] < 256 ? kRefineItems / a.P[l] : 256, tiles = (p.cap[l] + T - 1) / T;
            a.groups[l] = tiles < 1 ? 1 : (tiles < kRefineGroups ? tiles : kRefineGroups);
            if (o->level < 0 || o->level == l) width = a.groups[l] > width ? a.groups[l] : width;
            a.out0[l] = o->level < 0 ? at : 0;
            at += p.cap[l];
        }
        a.out_stride = o->level < 0 ? at : p.cap[o->level];
        a.g = d_g; a.h = d_h; a.cost = d_cost; a.valid = d_valid;
        a.out = (struct mbavo_pairs_refine *)refine_.p;
        a.partials = (double *)(refine_ + o_parts); a.tickets = (int *)(refine_ + o_tickets);
        const int rc = dispatch<2, 4>(k, [&](auto kd) {
            return dispatch<0, 1, 2>(p.format, [&](auto fmt) {
                auto kernel = k_pairs_refine<decltype(kd)::value, decltype(fmt)::value>;
                const hipError_t le = eng_.ensure_lds((const void *)kernel, lds);
                if (le != hipSuccess) return (int)le;
                hipLaunchKernelGGL(kernel, dim3(width, B * levels), dim3(256), lds, st, a);
                return 0;
            });
        });
        if (rc != 0) return rc;
        ref_stats_.launches = 1;
        if (!h_out) return (int)hipGetLastError(); // (nothing is waited for)
        return read_back(a.out, h_refine_, h_out, rec_bytes, ref_stats_);
    }
} // namespace mbavo

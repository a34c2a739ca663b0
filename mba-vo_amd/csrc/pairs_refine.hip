// pairs_refine.hip -- what the aligned blurred frame says about every keypoint's depth (include/mbavo.h: mbavo_pairs_refine_depths):
// per keypoint the gradient and Gauss-Newton curvature of its blur-aware patch cost with respect to its plane depth, the
// trajectory held at its estimate, and the damped inverse-depth step, optionally written in place.  ONE launch; a reported (pair,
// level) is served by G = min(kRefineGroups, ceil(capacity / T)) workgroups, workgroup g taking the tiles g, g + G, g + 2 G, .. of its
// keypoints (the grid is sized by the capacity, never by a count read back; a workgroup without a tile only hands in zeros).
//
// The evaluation -- prologue, items, the per-keypoint sums -- is pairs_depth_eval.h's depth_eval, shared with the depth filter
// (pairs_filter.hip); what is this kernel's own is its policy, RefineStep:
//
//   keypoint     the caller's per-keypoint arrays, the step, the optional store of the new depth, the lane's share of the record sums
//   record       butterfly within each wave, the four waves in order: the workgroup's four partial sums into scratch; the workgroup
//                that takes the LAST ticket of its (pair, level) adds the G partials in the order g = 0 .. G-1 and writes the record
#include "pairs_depth_eval.h"

namespace mbavo
{
    namespace pairs
    {
        struct RefineStep
        {
            const RefineArgs &a;
            mbavo_pairs_refine_opts o;
            double cost_sum = 0.0, rel_sum = 0.0;
            int n_full = 0, n_moved = 0;

            __device__ __forceinline__ explicit RefineStep(const RefineArgs &args) : a(args) {}

            __device__ __forceinline__ void off_knots(const DepthEvalSlot &c)
            {
                if (threadIdx.x == 0 && c.grp == 0)
                {
                    struct mbavo_pairs_refine *out = a.out + c.ent;
                    const double nan = __builtin_nan("");
                    out->status = MBAVO_E_RANGE; out->num_keypoints = c.K; out->num_full = 0; out->num_moved = 0;
                    out->cost = nan; out->sum_sq_rel = nan;
                }
            }

            __device__ __forceinline__ void begin(const DepthEvalSlot &) { o = *a.opts; }

            __device__ __forceinline__ void keypoint(const DepthEvalSlot &c, int kp, int nv, bool full, double g, double h, double cst)
            {
#pragma clang fp contract(off)
                if (a.g) a.g[c.o0 + kp] = g;
                if (a.h) a.h[c.o0 + kp] = h;
                if (a.cost) a.cost[c.o0 + kp] = cst;
                if (a.valid) a.valid[c.o0 + kp] = nv;
                if (!full) return;
                ++n_full;
                cost_sum = cost_sum + cst;
                const double D = c.kp_z[kp];
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
                        if (o.apply == 1) c.kp_z[kp] = D_new;
                    }
                }
            }

            // this workgroup's partial sums, then the last workgroup of the (pair, level) adds all G in group order
            __device__ __forceinline__ void finish(const DepthEvalSlot &c, double *s_w)
            {
                const double mine[4] = {cost_sum, rel_sum, (double)n_full, (double)n_moved}; // (integers below 2^53: exact)
                double r[4];
                if (!close_record<4>(mine, s_w, a.ev.partials, a.ev.tickets, c.ent, c.grp, c.G, r)) return;
                struct mbavo_pairs_refine *out = a.out + c.ent;
                out->status = 0; out->num_keypoints = c.K; out->num_full = (int)r[2]; out->num_moved = (int)r[3];
                out->cost = r[0]; out->sum_sq_rel = r[1];
            }
        };

        template <int KDEG, int GRAD>
        __global__ __launch_bounds__(256) void k_pairs_refine(const RefineArgs a)
        {
            extern __shared__ double s_dyn[]; // [S pose entries | the prologue's segments]
            __shared__ DepthEvalLds sh;
            RefineStep step(a);
            depth_eval<KDEG, GRAD>(a.ev, sh, s_dyn, step);
        }
    } // namespace pairs

    using namespace pairs;

    // What refinement, filter and search share on the host: the limits of this build on the reported levels (MBAVO_E_ARG), the
    // evaluation's arguments but for the record scratch, the grid's width and the dynamic LDS.
    int PairBatch::depth_eval_args(int level, DepthEvalArgs &a, int &width, size_t &lds) const
    {
        const PairsPlan &p = plan_;
        const int L = p.L, k = opts_.spline_deg_k;
        const int levels = level < 0 ? L : 1;
        lds = 0;
        for (int i = 0; i < levels; ++i)
        {
            const int l = level < 0 ? i : level;
            if (opts_.P[l] > kRefineItems) return MBAVO_E_ARG;
            const size_t need = k == 2 ? refine_lds<2>(opts_.S[l]) : refine_lds<4>(opts_.S[l]);
            lds = need > lds ? need : lds;
        }
        // (the static arrays: three doubles and a byte per item, the waves' sums, and what the bodies called keep: 25 888 B)
        if (lds + (size_t)kRefineItems * 25 + 512 > 160 * 1024) return MBAVO_E_ARG;
        a = DepthEvalArgs{};
        a.desc = lay_.desc(arena_); a.counts = lay_.counts(arena_); a.pattern = lay_.pattern(arena_);
        a.cap = lay_.cap(arena_); a.exp = lay_.exp(arena_); a.t0 = lay_.t0(arena_);
        a.kt = lay_.knots_t(arena_); a.kR = lay_.knots_R(arena_);
        a.of_pair = opts_.num_cameras > 0 ? lay_.pair_cameras(arena_) : nullptr;
        for (int i = 0; i < 4; ++i) a.intr[i] = opts_.intrinsics[i];
        a.dt = probs_[0].dt; a.huber_a = opts_.huber_a;
        a.L = L; a.N = p.N; a.level = level; a.levels = levels;
        for (int l = 0; l < L; ++l)
        {
            a.S[l] = opts_.S[l]; a.P[l] = opts_.P[l]; a.pat0[l] = p.pat0[l];
            a.groups[l] = DepthSlots::groups(p.cap[l], kRefineItems / a.P[l] < 256 ? kRefineItems / a.P[l] : 256);
        }
        width = DepthSlots::width(level, a.groups);
        a.out_stride = slots_.outs(level, a.out0);
        return 0;
    }

    int PairBatch::refine_depths(const mbavo_pairs_refine_opts *o, struct mbavo_pairs_refine *h_out, double *d_g, double *d_h, double *d_cost,
                                 int *d_valid)
    {
        DepthCall &call = refine_call_;
        call.stats = CallStats{};
        if (!arena_ || !prepared_ || !motion_set_ || !o) return MBAVO_E_ARG;
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L, k = opts_.spline_deg_k;
        mbavo_pairs_refine_opts opt;
        if (depth_step_opts(o, L, opt) != 0) return MBAVO_E_ARG;
        const int levels = o->level < 0 ? L : 1;
        RefineArgs a{};
        int width;
        size_t lds;
        if (depth_eval_args(o->level, a.ev, width, lds) != 0) return MBAVO_E_ARG;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        const size_t rec = sizeof(struct mbavo_pairs_refine) * (size_t)B, opt_bytes = sizeof(mbavo_pairs_refine_opts);
        if ((e = call.open(rec * L, 4, opt_bytes)) != hipSuccess) return (int)e;
        *(mbavo_pairs_refine_opts *)call.h_opts = opt;
        if ((e = call.upload(opt_bytes)) != hipSuccess) return (int)e;
        a.opts = (const mbavo_pairs_refine_opts *)call.d_opts;
        a.g = d_g; a.h = d_h; a.cost = d_cost; a.valid = d_valid;
        a.out = (struct mbavo_pairs_refine *)call.records;
        a.ev.partials = call.partials; a.ev.tickets = call.tickets;
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
        call.stats.launches = 1;
        return call.finish(h_out, rec * levels);
    }
} // namespace mbavo

// pairs_search.hip -- the exhaustive counterpart of the depth refinement (include/mbavo.h: mbavo_pairs_search_depths): the blur-aware
// patch cost of every keypoint at ND inverse-depth candidates, the patch centre in the blurred frame moving with the candidate --
// the epipolar search on the blurred image along the estimated in-exposure trajectory -- and per keypoint the best candidate with
// a sub-candidate parabola fit, a curvature and a runner-up.  ONE launch on the refinement's grid.
//
// The evaluation -- prologue, the cost-only item, the per-keypoint sums over kSearchBatch candidates per barrier pair -- is
// pairs_depth_eval.h's depth_search; what is this kernel's own is its policy, SearchStep:
//
//   candidate    a streaming selection in the keypoint's lane, no ND-long array: the four lowest (cost, index) pairs sorted, ties
//                to the lower index (at most two candidates are adjacent to the best one, so the lowest non-adjacent of the other
//                three is the runner-up of all); the previous candidate's cost, which becomes c_- when a new best arrives; c_+
//                captured at d == best + 1
//   keypoint     parabola, acceptance, the caller's per-keypoint arrays, the optional store of the new depth, the lane's share of
//                the record sums
//   record       four sums, closed as the refinement closes its four (close_record)
#include "pairs_depth_eval.h"

namespace mbavo
{
    namespace pairs
    {
        struct SearchStep
        {
            const SearchArgs &a;
            mbavo_pairs_search_opts o;
            double kc[4], prev, c_minus, c_plus; // the four lowest costs in order; costs of d - 1, best - 1, best + 1 (NaN: not full, or none)
            int ki[4], n_cand;                   // their candidates (-1: none yet); full candidates so far
            double cost_sum = 0.0, ratio_sum = 0.0;
            int n_searched = 0, n_accepted = 0;

            __device__ __forceinline__ explicit SearchStep(const SearchArgs &args) : a(args) {}

            __device__ __forceinline__ void off_knots(const DepthEvalSlot &c)
            {
                if (threadIdx.x == 0 && c.grp == 0)
                {
                    struct mbavo_pairs_search *out = a.out + c.ent;
                    const double nan = __builtin_nan("");
                    out->status = MBAVO_E_RANGE; out->num_keypoints = c.K; out->num_searched = 0; out->num_accepted = 0;
                    out->cost = nan; out->sum_ratio = nan;
                }
            }

            __device__ __forceinline__ void begin(const DepthEvalSlot &) { o = *a.opts; }

            __device__ __forceinline__ int candidates() const { return o.num_candidates; }

            // step 1: rho_0 and the spacing of the candidates of a keypoint at depth D
            __device__ __forceinline__ void range(double D, double &lo, double &st) const
            {
#pragma clang fp contract(off)
                lo = o.rho_lo;
                double hi = o.rho_hi;
                if (o.relative == 1)
                {
                    lo = o.rho_lo / D;
                    hi = o.rho_hi / D;
                }
                st = (hi - lo) / (double)(o.num_candidates - 1);
            }

            __device__ __forceinline__ void candidate(const DepthEvalSlot &c, int kp, int d, double cost)
            {
                if (d == 0)
                {
                    const double inf = __builtin_inf(), nan = __builtin_nan("");
#pragma unroll
                    for (int i = 0; i < 4; ++i) { kc[i] = inf; ki[i] = -1; }
                    prev = nan; c_minus = nan; c_plus = nan;
                    n_cand = 0;
                }
                if (a.volume) a.volume[(c.o0 + kp) * o.num_candidates + d] = cost;
                if (ki[0] >= 0 && d == ki[0] + 1) c_plus = cost;
                if (cost == cost)
                { // a full candidate: into the sorted four, behind every entry that costs the same
                    ++n_cand;
                    double cc = cost;
                    int ci = d;
                    bool moving = false;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (moving || cc < kc[i])
                        {
                            const double tc = kc[i];
                            const int ti = ki[i];
                            kc[i] = cc; ki[i] = ci;
                            cc = tc; ci = ti;
                            moving = true;
                        }
                    if (ki[0] == d)
                    { // a new best: its lower neighbour is the candidate before it, its upper one is still to come
                        c_minus = prev;
                        c_plus = __builtin_nan("");
                    }
                }
                prev = cost;
            }

            // steps 3 - 5 on what the candidates left
            __device__ __forceinline__ void keypoint(const DepthEvalSlot &c, int kp)
            {
#pragma clang fp contract(off)
                const double nan = __builtin_nan("");
                const int best = ki[0], ND = o.num_candidates;
                double second = nan;
#pragma unroll
                for (int i = 3; i >= 1; --i)
                    if (ki[i] >= 0 && (ki[i] - best > 1 || best - ki[i] > 1)) second = kc[i];
                double lo, st;
                range(c.kp_z[kp], lo, st);
                double rho = nan, curv = 0.0, cost_best = nan;
                bool parabola = false;
                if (best >= 0)
                {
                    cost_best = kc[0];
                    rho = lo + (double)best * st;
                    if (best > 0 && best < ND - 1 && c_minus == c_minus && c_plus == c_plus)
                    {
                        const double den = (c_minus - 2.0 * cost_best) + c_plus;
                        if (den > 0.0)
                        {
                            double delta = 0.5 * (c_minus - c_plus) / den;
                            if (delta > 0.5) delta = 0.5;
                            if (delta < -0.5) delta = -0.5;
                            rho = rho + delta * st;
                            curv = den / (st * st);
                            parabola = true;
                        }
                    }
                }
                const long long at = c.o0 + kp;
                if (a.rho) a.rho[at] = rho;
                if (a.cost_best) a.cost_best[at] = cost_best;
                if (a.cost_second) a.cost_second[at] = second;
                if (a.curv) a.curv[at] = curv;
                if (a.best) a.best[at] = best;
                if (a.num_full) a.num_full[at] = n_cand;
                if (best < 0) return;
                ++n_searched;
                if (o.min_ratio != 0.0 && !(second >= o.min_ratio * cost_best)) return; // (a NaN runner-up fails)
                if (parabola ? !(curv > o.min_curv) : o.min_curv != 0.0) return;
                const double D_new = 1.0 / rho;
                if (!(__builtin_isfinite(D_new) && D_new >= o.z_min && (o.z_max == 0.0 || D_new <= o.z_max))) return;
                ++n_accepted;
                cost_sum = cost_sum + cost_best;
                if (second == second && second != 0.0) ratio_sum = ratio_sum + cost_best / second;
                if (o.apply == 1) c.kp_z[kp] = D_new;
            }

            // this workgroup's partial sums, then the last workgroup of the (pair, level) adds all G in group order
            __device__ __forceinline__ void finish(const DepthEvalSlot &c, double *s_w)
            {
                const double mine[4] = {cost_sum, ratio_sum, (double)n_searched, (double)n_accepted}; // (integers below 2^53: exact)
                double r[4];
                if (!close_record<4>(mine, s_w, a.ev.partials, a.ev.tickets, c.ent, c.grp, c.G, r)) return;
                struct mbavo_pairs_search *out = a.out + c.ent;
                out->status = 0; out->num_keypoints = c.K; out->num_searched = (int)r[2]; out->num_accepted = (int)r[3];
                out->cost = r[0]; out->sum_ratio = r[1];
            }
        };

        template <int KDEG>
        __global__ __launch_bounds__(256) void k_pairs_search(const SearchArgs a)
        {
            extern __shared__ double s_dyn[]; // [S pose entries | the prologue's segments]
            __shared__ DepthSearchLds sh;
            SearchStep step(a);
            depth_search<KDEG>(a.ev, sh, s_dyn, step);
        }
    } // namespace pairs

    using namespace pairs;

    // (follows refine_depths where the two agree: the checks, the call, the dispatch)
    int PairBatch::search_depths(const mbavo_pairs_search_opts *o, struct mbavo_pairs_search *h_out, double *d_rho, double *d_cost_best,
                                 double *d_cost_second, double *d_curv, int *d_best, int *d_num_full, double *d_volume)
    {
        DepthCall &call = search_call_;
        call.stats = CallStats{};
        if (!arena_ || !prepared_ || !motion_set_ || !o) return MBAVO_E_ARG;
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L, k = opts_.spline_deg_k;
        if (o->level < -1 || o->level >= L || !flags01({o->apply, o->relative})) return MBAVO_E_ARG;
        if (o->num_candidates < 2 || o->num_candidates > 64) return MBAVO_E_ARG;
        if (bad_limit(o->rho_lo) || bad_limit(o->rho_hi) || bad_limit(o->min_ratio) || bad_limit(o->min_curv)) return MBAVO_E_ARG;
        if (!(0.0 < o->rho_lo && o->rho_lo < o->rho_hi) || (o->min_ratio != 0.0 && o->min_ratio < 1.0)) return MBAVO_E_ARG;
        mbavo_pairs_search_opts opt = *o;
        if (depth_limits(opt.z_min, opt.z_max) != 0) return MBAVO_E_ARG;
        const int levels = o->level < 0 ? L : 1;
        SearchArgs a{};
        int width;
        size_t lds;
        if (depth_eval_args(o->level, a.ev, width, lds) != 0) return MBAVO_E_ARG;
        if (lds + sizeof(DepthSearchLds) + 512 > 160 * 1024) return MBAVO_E_ARG; // (the kernel's static LDS: 33 056 B)
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        const size_t rec = sizeof(struct mbavo_pairs_search) * (size_t)B, opt_bytes = sizeof(mbavo_pairs_search_opts);
        if ((e = call.open(rec * L, 4, opt_bytes)) != hipSuccess) return (int)e;
        *(mbavo_pairs_search_opts *)call.h_opts = opt;
        if ((e = call.upload(opt_bytes)) != hipSuccess) return (int)e;
        a.opts = (const mbavo_pairs_search_opts *)call.d_opts;
        a.rho = d_rho; a.cost_best = d_cost_best; a.cost_second = d_cost_second; a.curv = d_curv; a.volume = d_volume;
        a.best = d_best; a.num_full = d_num_full;
        a.out = (struct mbavo_pairs_search *)call.records;
        a.ev.partials = call.partials; a.ev.tickets = call.tickets;
        const int rc = dispatch<2, 4>(k, [&](auto kd) { // (no gradient taps: the keyframe's format makes no difference to the kernel)
            auto kernel = k_pairs_search<decltype(kd)::value>;
            const hipError_t le = eng_.ensure_lds((const void *)kernel, lds);
            if (le != hipSuccess) return (int)le;
            hipLaunchKernelGGL(kernel, dim3(width, B * levels), dim3(256), lds, st, a);
            return 0;
        });
        if (rc != 0) return rc;
        call.stats.launches = 1;
        return call.finish(h_out, rec * levels);
    }
} // namespace mbavo

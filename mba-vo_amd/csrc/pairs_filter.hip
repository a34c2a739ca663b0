// pairs_filter.hip -- the recursive inverse-depth filter of every keypoint over the frames that track its keyframe (include/mbavo.h:
// mbavo_pairs_filter_depths): what the aligned blurred frame says about a keypoint's depth -- the refinement's g and h, from the
// same device bodies (pairs_depth_eval.h: depth_eval) -- fused with the keypoint's mean inverse depth and information kept on the
// device, behind an innovation gate, and the fused depth optionally written in place.  ONE launch on the refinement's grid.
//
// What is this kernel's own is its policy, FilterStep:
//
//   seed         a (pair, level) whose keypoints were rewritten since its state was last seeded (the host keeps a serial per pair
//                and uploads one word of level bits per pair behind the options), or any under reset = 1: mu = 1 / D, info from
//                the prior, counters zero -- in the keypoint's own lane, in place of the state's load; a pair off its knots is
//                seeded all the same, by the lanes that would have served its tiles
//   keypoint     the state of keypoint kp at [pair b's Σcap | level l's offset | kp] of four arrays (a lane per keypoint:
//                consecutive addresses), gate, fusion, the optional store of the new depth, the lane's share of the record sums
//   record       six sums, closed as the refinement closes its four (close_record)
#include "pairs_depth_eval.h"

namespace mbavo
{
    namespace pairs
    {
        constexpr int kFilterSums = 6; // cost, sum_info, sum_sq_rel, num_full, num_fused, num_rejected

        struct FilterStep
        {
            const FilterArgs &a;
            mbavo_pairs_filter_opts o;
            long long s0 = 0; // the (pair, level)'s first state entry
            bool seed = false;
            double cost_sum = 0.0, info_sum = 0.0, rel_sum = 0.0;
            int n_full = 0, n_fused = 0, n_rejected = 0;

            __device__ __forceinline__ explicit FilterStep(const FilterArgs &args) : a(args) {}

            __device__ __forceinline__ void slot(const DepthEvalSlot &c)
            {
                o = *a.opts;
                s0 = (long long)c.b * a.st_stride + a.st0[c.l];
                seed = ((a.seed[c.b] >> c.l) & 1) != 0;
            }

            __device__ __forceinline__ void seed_values(double D, double &mu, double &info) const
            {
#pragma clang fp contract(off)
                mu = 1.0 / D;
                info = o.prior_rel_sigma == 0.0 ? 0.0 : 1.0 / ((o.prior_rel_sigma * mu) * (o.prior_rel_sigma * mu));
            }

            // no pose, no measurement: the seed alone, by the lanes of the tiles this workgroup would have served
            __device__ __forceinline__ void off_knots(const DepthEvalSlot &c)
            {
                slot(c);
                if (seed)
                    for (int tile = c.grp * c.T; tile < c.K; tile += c.G * c.T)
                    {
                        const int kp = tile + (int)threadIdx.x;
                        if ((int)threadIdx.x < c.T && kp < c.K)
                        {
                            double mu, info;
                            seed_values(c.kp_z[kp], mu, info);
                            a.mu[s0 + kp] = mu; a.info[s0 + kp] = info;
                            a.n_obs[s0 + kp] = 0; a.n_rej[s0 + kp] = 0;
                        }
                    }
                if (threadIdx.x == 0 && c.grp == 0)
                {
                    struct mbavo_pairs_filter *out = a.out + c.ent;
                    const double nan = __builtin_nan("");
                    out->status = MBAVO_E_RANGE; out->num_keypoints = c.K; out->num_full = 0; out->num_fused = 0; out->num_rejected = 0;
                    out->seeded = seed ? 1 : 0;
                    out->cost = nan; out->sum_info = nan; out->sum_sq_rel = nan;
                }
            }

            __device__ __forceinline__ void begin(const DepthEvalSlot &c) { slot(c); }

            __device__ __forceinline__ void keypoint(const DepthEvalSlot &c, int kp, int, bool full, double g, double h, double cst)
            {
#pragma clang fp contract(off)
                const long long si = s0 + kp;
                const double D = c.kp_z[kp];
                double mu, info;
                int n_obs = 0, n_rej = 0;
                if (seed) seed_values(D, mu, info);
                else
                {
                    mu = a.mu[si]; info = a.info[si];
                    n_obs = a.n_obs[si]; n_rej = a.n_rej[si];
                }
                bool dirty = seed;
                if (full)
                {
                    ++n_full;
                    cost_sum = cost_sum + cst;
                    const double s2 = o.sigma_i * o.sigma_i;
                    const double rho_c = 1.0 / D, DD = D * D;
                    const double g_rho = -(DD * g), h_rho = (DD * DD) * h;
                    const double hm = h_rho / s2;
                    if (hm > o.min_info && h_rho > 0.0)
                    {
                        bool rejected = false;
                        if (o.gate_chi2 > 0.0 && info > 0.0)
                        {
                            const double rho_m = rho_c - g_rho / h_rho;
                            const double e = rho_m - mu;
                            const double c2 = (e * e) * ((info * hm) / (info + hm));
                            rejected = c2 > o.gate_chi2;
                        }
                        if (rejected)
                        {
                            ++n_rej; ++n_rejected;
                            dirty = true;
                        }
                        else
                        {
                            const double A = info + hm;
                            const double bv = info * (mu - rho_c) - g_rho / s2;
                            const double m = o.max_rel_step * rho_c;
                            double d_rho = bv / A;
                            if (d_rho > m) d_rho = m;
                            if (d_rho < -m) d_rho = -m;
                            const double rho_n = rho_c + d_rho;
                            const double D_new = 1.0 / rho_n;
                            if (__builtin_isfinite(D_new) && D_new >= o.z_min && (o.z_max == 0.0 || D_new <= o.z_max))
                            {
                                const double rel = d_rho / rho_c;
                                mu = rho_n; info = A; ++n_obs;
                                dirty = true;
                                ++n_fused;
                                info_sum = info_sum + A;
                                rel_sum = rel_sum + rel * rel;
                                if (o.apply == 1) c.kp_z[kp] = D_new;
                            }
                        }
                    }
                }
                if (dirty)
                {
                    a.mu[si] = mu; a.info[si] = info;
                    a.n_obs[si] = n_obs; a.n_rej[si] = n_rej;
                }
            }

            __device__ __forceinline__ void finish(const DepthEvalSlot &c, double *s_w)
            {
                const double mine[kFilterSums] = {cost_sum, info_sum, rel_sum, (double)n_full, (double)n_fused, (double)n_rejected}; // (integers below 2^53: exact)
                double r[kFilterSums];
                if (!close_record<kFilterSums>(mine, s_w, a.ev.partials, a.ev.tickets, c.ent, c.grp, c.G, r)) return;
                struct mbavo_pairs_filter *out = a.out + c.ent;
                out->status = 0; out->num_keypoints = c.K; out->num_full = (int)r[3]; out->num_fused = (int)r[4]; out->num_rejected = (int)r[5];
                out->seeded = seed ? 1 : 0;
                out->cost = r[0]; out->sum_info = r[1]; out->sum_sq_rel = r[2];
            }
        };

        template <int KDEG, int GRAD>
        __global__ __launch_bounds__(256) void k_pairs_filter(const FilterArgs a)
        {
            extern __shared__ double s_dyn[]; // [S pose entries | the prologue's segments]
            __shared__ DepthEvalLds sh;
            FilterStep step(a);
            depth_eval<KDEG, GRAD>(a.ev, sh, s_dyn, step);
        }
    } // namespace pairs

    using namespace pairs;

    // (follows refine_depths where the two agree: the checks, the call, the dispatch)
    int PairBatch::filter_depths(const mbavo_pairs_filter_opts *o, struct mbavo_pairs_filter *h_out)
    {
        DepthCall &call = filter_call_;
        call.stats = CallStats{};
        if (!arena_ || !prepared_ || !motion_set_ || !o) return MBAVO_E_ARG;
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L, k = opts_.spline_deg_k;
        mbavo_pairs_filter_opts opt;
        if (depth_step_opts(o, L, opt) != 0) return MBAVO_E_ARG;
        if (bad_limit(o->sigma_i) || bad_limit(o->prior_rel_sigma) || bad_limit(o->gate_chi2) || !flags01({o->reset})) return MBAVO_E_ARG;
        if (opt.sigma_i == 0.0) opt.sigma_i = 1.0;
        const int levels = o->level < 0 ? L : 1;
        FilterArgs a{};
        int width;
        size_t lds;
        if (depth_eval_args(o->level, a.ev, width, lds) != 0) return MBAVO_E_ARG;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        const size_t rec = sizeof(struct mbavo_pairs_filter) * (size_t)B;
        const size_t opt_bytes = sizeof(mbavo_pairs_filter_opts) + sizeof(int) * (size_t)B; // the options and the B seed words: ONE copy
        // the first call: the state and the scratch (include/mbavo.h)
        if (!call.dev)
        {
            if (!filter_state_)
            {
                if ((e = filter_state_.alloc(slots_.n_slots * 24 + 8)) != hipSuccess) return (int)e;
                if ((e = hipMemsetAsync(filter_state_.p, 0, slots_.n_slots * 24 + 8, st)) != hipSuccess) return (int)e;
            }
            seeded_at_.assign((size_t)B * L, 0);
        }
        if ((e = call.open(rec * L, kFilterSums, opt_bytes)) != hipSuccess) return (int)e;
        mbavo_pairs_filter_opts *h_opts = (mbavo_pairs_filter_opts *)call.h_opts;
        int *h_seed = (int *)(h_opts + 1);
        *h_opts = opt;
        for (int b = 0; b < B; ++b)
        { // bit l: level l of pair b is reported and its keypoints are not the ones its state was seeded from
            int word = 0;
            for (int i = 0; i < levels; ++i)
            {
                const int l = o->level < 0 ? i : o->level;
                if (o->reset == 1 || seeded_at_[(size_t)b * L + l] != kp_serial_[b]) word |= 1 << l;
            }
            h_seed[b] = word;
        }
        if ((e = call.upload(opt_bytes)) != hipSuccess) return (int)e;
        a.opts = (const mbavo_pairs_filter_opts *)call.d_opts; a.seed = (const int *)(a.opts + 1);
        const FilterArrays f = filter_arrays();
        a.mu = f.mu; a.info = f.info; a.n_obs = f.n_obs; a.n_rej = f.n_rej;
        a.st_stride = slots_.outs(-1, a.st0); // (the state is in the layout of level = -1 whatever the call's level is)
        a.out = (struct mbavo_pairs_filter *)call.records;
        a.ev.partials = call.partials; a.ev.tickets = call.tickets;
        const int rc = dispatch<2, 4>(k, [&](auto kd) {
            return dispatch<0, 1, 2>(p.format, [&](auto fmt) {
                auto kernel = k_pairs_filter<decltype(kd)::value, decltype(fmt)::value>;
                const hipError_t le = eng_.ensure_lds((const void *)kernel, lds);
                if (le != hipSuccess) return (int)le;
                hipLaunchKernelGGL(kernel, dim3(width, B * levels), dim3(256), lds, st, a);
                return 0;
            });
        });
        if (rc != 0) return rc;
        call.stats.launches = 1;
        filter_ready_ = true;
        for (int b = 0; b < B; ++b) // (the launch seeds them, on or off the knots)
            for (int l = 0; l < L; ++l)
                if ((h_seed[b] >> l) & 1) seeded_at_[(size_t)b * L + l] = kp_serial_[b];
        return call.finish(h_out, rec * levels);
    }

    int PairBatch::filter_state(double **d_mu, double **d_info, int **d_n_obs, int **d_n_rej, long long *h_pair_stride, long long h_level_offset[8]) const
    {
        if (!filter_ready_ || !d_mu || !d_info || !d_n_obs || !d_n_rej || !h_pair_stride || !h_level_offset) return MBAVO_E_ARG;
        *h_pair_stride = slots_.outs(-1, h_level_offset);
        const FilterArrays f = filter_arrays();
        *d_mu = f.mu; *d_info = f.info; *d_n_obs = f.n_obs; *d_n_rej = f.n_rej;
        return 0;
    }
} // namespace mbavo

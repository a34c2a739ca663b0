// pairs_hyp.hip -- every pair's start picked among M motion hypotheses (include/mbavo.h: mbavo_pairs_predict_hypotheses), in
// predict's place in the frame:
//
//   k_pairs_hypotheses   a workgroup per pair, a lane per (hypothesis, knot): dT_m = exp((scale_m velocity) dt_frame + twist_m)
//                        once per hypothesis, every knot through TransformByRight into the candidates; the times published and
//                        dt_frame kept as k_pairs_predict does
//   the evaluation       ONE cost-only evaluation of the B * M candidate entries (the engine's, unchanged)
//   k_pairs_hyp_select   16 lanes per pair: the score per in-bounds pixel, eligibility, the winner, its knots into the knots the
//                        problems point at, the record
//
// Hypothesis 0 restates k_pairs_predict (pairs_track.hip) expression for expression, with the device functions it uses, so that its
// candidate has the predict's bits; the two kernels are separate because the candidates of a pair fill a workgroup here.
#include "pairs_prep.h"
#include "pairs_desc.h"
#include "pose_math.h"
#include "se3_math.h"
#include <cmath>
#include <cstring>
#include <hip/hip_runtime.h>

namespace mbavo
{
    namespace pairs
    {
        constexpr int kMaxHyp = MBAVO_PAIRS_MAX_HYP;
        static_assert(kMaxHyp == 16, "a workgroup of 256 holds 16 hypotheses x 16 knots");

        // lane = 16 m + i: hypothesis m, knot i.  The first lane of a hypothesis forms dT_m into LDS; one barrier; lane (m, i) moves
        // knot i by dT_m into candidate (b, m).  The pair's own knots are only read.  Lane 0 does what k_pairs_predict's first lane
        // does besides: dt_frame into the state, cap / exp / t0 published.
        __global__ __launch_bounds__(256) void k_pairs_hypotheses(const HypArgs p)
        {
            __shared__ double s_dT[kMaxHyp][7];
            const int b = (int)blockIdx.x, m = threadIdx.x >> 4, i = threadIdx.x & 15;
            const int M = p.opts->M, N = p.N;
            if (m < M && i == 0)
            {
#pragma clang fp contract(off)
                double *st = p.state + (size_t)b * kStateLen;
                const double cap = p.times[b], ex = p.times[p.B + b], t0 = p.times[2 * p.B + b];
                const double dt_frame = cap - st[kStatePrevTime];
                double v[6], dT[7];
                if (m == 0)
                {
#pragma unroll
                    for (int j = 0; j < 6; ++j) v[j] = st[kStateVelocity + j] * dt_frame;
                }
                else
                {
                    const double s = p.opts->scale[m];
#pragma unroll
                    for (int j = 0; j < 6; ++j) v[j] = (s * st[kStateVelocity + j]) * dt_frame + p.opts->twist[m][j];
                }
                se3_exp(v, dT);
#pragma unroll
                for (int j = 0; j < 7; ++j) s_dT[m][j] = dT[j];
                if (m == 0)
                { // (no lane reads what these stores write)
                    st[kStateDtFrame] = dt_frame;
                    p.cap[b] = cap; p.exp[b] = ex; p.t0[b] = t0;
                }
            }
            __syncthreads();
            if (m < M && i < N)
            { // SplineSE3::TransformByRight on knot i
#pragma clang fp contract(off)
                const double *kt = p.kt + ((size_t)b * N + i) * 3, *kR = p.kR + ((size_t)b * N + i) * 4;
                const size_t e = (size_t)b * M + m;
                double *ct = p.cand_t + (e * N + i) * 3, *cR = p.cand_R + (e * N + i) * 4;
                const double d[3] = {s_dT[m][0], s_dT[m][1], s_dT[m][2]};
                const Quat dq{s_dT[m][3], s_dT[m][4], s_dT[m][5], s_dT[m][6]}, R = load_quat(kR);
                double r[3];
                qrotate(R, d, r);
                ct[0] = kt[0] + r[0]; ct[1] = kt[1] + r[1]; ct[2] = kt[2] + r[2];
                const Quat n = qmul(R, dq);
                cR[0] = n.x; cR[1] = n.y; cR[2] = n.z; cR[3] = n.w;
            }
        }

        // 16 lanes per pair, 16 pairs per workgroup.  Lane m scores hypothesis m; the pair's first lane walks the scores in index
        // order (the lowest index wins a tie) and writes the record's head; lane i < N copies knot i of the winner.  A pair reads
        // nothing of another's and nothing is accumulated: the same bits from run to run and for any B.
        __global__ __launch_bounds__(256) void k_pairs_hyp_select(const HypSelectArgs a)
        {
#pragma clang fp contract(off)
            __shared__ double s_score[16][kMaxHyp];
            __shared__ int s_elig[16][kMaxHyp], s_win[16];
            const int g = threadIdx.x >> 4, i = threadIdx.x & 15, b = (int)blockIdx.x * 16 + g;
            const bool live = b < a.B;
            const int M = a.opts->M, N = a.N;
            const int K = live ? a.counts[(size_t)b * a.L + a.opts->level] : 0;
            const double KP = (double)K * (double)a.P;
            double score = 0.0, valid = 0.0;
            int elig = 0;
            if (live && i < M)
            {
                const size_t e = (size_t)b * M + i;
                const double cost = a.blocks[e * a.E];
                valid = a.valid[e];
                score = (cost * KP) / valid;
                elig = (K > 0 && valid >= a.opts->min_valid_frac * KP && __builtin_isfinite(score)) ? 1 : 0;
            }
            s_score[g][i] = score;
            s_elig[g][i] = elig;
            __syncthreads();
            if (live && i == 0)
            {
                int c = -1, n = s_elig[g][0];
                for (int m = 1; m < M; ++m)
                {
                    if (!s_elig[g][m]) continue;
                    ++n;
                    if (c < 0 || s_score[g][m] < s_score[g][c]) c = m;
                }
                int w = 0;
                if (c >= 0 && (!s_elig[g][0] || s_score[g][c] < s_score[g][0] * (1.0 - a.opts->min_gain))) w = c;
                mbavo_pairs_hyp *o = a.out + b;
                o->winner = w; o->status = n == 0 ? MBAVO_HYP_NONE_ELIGIBLE : 0; o->num_keypoints = K; o->num_eligible = n;
                s_win[g] = w;
            }
            __syncthreads();
            if (!live) return;
            mbavo_pairs_hyp *o = a.out + b;
            o->score[i] = score; // (lanes >= M: 0)
            o->valid[i] = valid;
            if (i < N)
            {
                const size_t e = (size_t)b * M + s_win[g];
                const double *ct = a.cand_t + (e * N + i) * 3, *cR = a.cand_R + (e * N + i) * 4;
                double *kt = a.kt + ((size_t)b * N + i) * 3, *kR = a.kR + ((size_t)b * N + i) * 4;
                kt[0] = ct[0]; kt[1] = ct[1]; kt[2] = ct[2];
                kR[0] = cR[0]; kR[1] = cR[1]; kR[2] = cR[2]; kR[3] = cR[3];
            }
        }
    } // namespace pairs

    using namespace pairs;

    int PairBatch::predict_hypotheses(const double *h_cap, const double *h_exp, const mbavo_pairs_hyp_opts *o, mbavo_pairs_hyp *h_out)
    {
        if (!arena_ || !prepared_ || !states_set_ || pending_ || !h_cap || !h_exp || !o) return MBAVO_E_ARG;
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L, N = p.N, k = opts_.spline_deg_k, nd = 6 * k + 1, E = nd * (nd + 1) / 2;
        const int M = o->M;
        if (M < 1 || M > kMaxHyp || o->level < 0 || o->level >= L) return MBAVO_E_ARG;
        if (!std::isfinite(o->min_valid_frac) || o->min_valid_frac < 0.0 || o->min_valid_frac > 1.0) return MBAVO_E_ARG;
        if (!std::isfinite(o->min_gain) || o->min_gain < 0.0 || !(o->min_gain < 1.0)) return MBAVO_E_ARG;
        for (int m = 1; m < M; ++m)
        {
            if (!std::isfinite(o->scale[m])) return MBAVO_E_ARG;
            for (int j = 0; j < 6; ++j)
                if (!std::isfinite(o->twist[m][j])) return MBAVO_E_ARG;
        }
        const double dt = state_dt_;
        // the times are the same for every hypothesis: predict's own host check, nothing touched before every pair has passed
        if (!samples_on_knots(h_cap, h_exp, nullptr, dt)) return MBAVO_E_RANGE;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        const size_t rec_bytes = sizeof(mbavo_pairs_hyp) * (size_t)B, opt_bytes = sizeof(mbavo_pairs_hyp_opts);
        const long long slots = (long long)B * kMaxHyp;
        const long long o_cand_R = align_up((long long)sizeof(double) * slots * 3 * N, kAlign);
        const long long o_blocks = o_cand_R + align_up((long long)sizeof(double) * slots * 4 * N, kAlign);
        const long long o_valid = o_blocks + align_up((long long)sizeof(double) * slots * E, kAlign);
        const long long o_rec = o_valid + align_up((long long)sizeof(double) * slots, kAlign);
        const long long o_opts = o_rec + align_up((long long)rec_bytes, kAlign);
        // the first call: its scratch (include/mbavo.h)
        if (!h_hyp_ && (e = h_hyp_.alloc(rec_bytes + opt_bytes)) != hipSuccess) return (int)e;
        if (!hyp_ && (e = hyp_.alloc((size_t)o_opts + opt_bytes)) != hipSuccess) return (int)e;
        hyp_probs_.reserve((size_t)slots);
        hyp_stats_ = CallStats{};
        // (the options' mirror is free as h_times_ is: the last copy out of it was followed by a commit, a set_states or this
        // call's own synchronisation)
        if ((e = upload_times(h_cap, h_exp)) != hipSuccess) return (int)e;
        mbavo_pairs_hyp_opts *h_opts = (mbavo_pairs_hyp_opts *)(h_hyp_ + rec_bytes);
        *h_opts = *o;
        if (h_opts->min_valid_frac == 0.0) h_opts->min_valid_frac = 0.5;
        const mbavo_pairs_hyp_opts *d_opts = (const mbavo_pairs_hyp_opts *)(hyp_ + o_opts);
        if ((e = hipMemcpyAsync((void *)d_opts, h_opts, opt_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        double *kt = lay_.knots_t(arena_), *kR = lay_.knots_R(arena_);
        double *cand_t = (double *)hyp_.p, *cand_R = (double *)(hyp_ + o_cand_R);
        double *blocks = (double *)(hyp_ + o_blocks), *valid = (double *)(hyp_ + o_valid);
        HypArgs h;
        h.state = lay_.state(arena_);
        h.kt = kt; h.kR = kR;
        h.cap = lay_.cap(arena_); h.exp = lay_.exp(arena_); h.t0 = lay_.t0(arena_);
        h.times = lay_.times(arena_);
        h.opts = d_opts;
        h.cand_t = cand_t; h.cand_R = cand_R;
        h.B = B; h.N = N;
        hipLaunchKernelGGL(k_pairs_hypotheses, dim3(B), dim3(256), 0, st, h);
        hyp_stats_.launches = 1;
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        publish_times(h_cap, h_times_ + 2 * B, dt);
        motion_set_ = true; // (the times are all there, and after the selection the knots)
        // entry (b, m): pair b's entry of the level, on candidate (b, m), with no keypoint excluded
        hyp_probs_.resize((size_t)B * M);
        for (int b = 0; b < B; ++b)
            for (int m = 0; m < M; ++m)
            {
                const size_t i = (size_t)b * M + m;
                mbavo_problem &q = hyp_probs_[i];
                q = probs_[(size_t)b * L + o->level];
                q.d_knots_t = cand_t + i * 3 * N; q.d_knots_R = cand_R + i * 4 * N;
                q.d_outlier = nullptr; q.num_bad = 0; q.num_residuals = 0;
            }
        const int rc = eng_.evaluate(B * M, hyp_probs_.data(), k, false, blocks, nullptr, valid, nullptr);
        if (rc != 0)
        { // no predict is pending: mbavo_pairs_set_states starts over
            (void)hipStreamSynchronize(st);
            return rc;
        }
        hyp_stats_.launches += evaluation_launches(eng_);
        HypSelectArgs s;
        s.counts = lay_.counts(arena_);
        s.blocks = blocks; s.valid = valid;
        s.cand_t = cand_t; s.cand_R = cand_R;
        s.kt = kt; s.kR = kR;
        s.opts = d_opts;
        s.out = (mbavo_pairs_hyp *)(hyp_ + o_rec);
        s.B = B; s.L = L; s.N = N; s.E = E; s.P = opts_.P[o->level];
        hipLaunchKernelGGL(k_pairs_hyp_select, dim3((B + 15) / 16), dim3(256), 0, st, s);
        ++hyp_stats_.launches;
        if ((e = hipGetLastError()) != hipSuccess)
        {
            (void)hipStreamSynchronize(st);
            return (int)e;
        }
        pending_ = true;
        if (!h_out) return 0; // (nothing is waited for, as in predict)
        return read_back(s.out, h_hyp_, h_out, rec_bytes, hyp_stats_);
    }
} // namespace mbavo

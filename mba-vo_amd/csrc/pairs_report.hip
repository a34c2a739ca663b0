// pairs_report.hip -- how far the pose of a pair can be trusted (include/mbavo.h: mbavo_pairs_report): behind an alignment, one
// level-0 evaluation of all B pairs with no keypoint excluded (the engine's, unchanged) and ONE launch that turns every pair's
// packed frame block, knots and patch costs into a record -- a workgroup per pair:
//
//   A            the 6k x 6 matrix that maps a rigid shift (v, w) of the whole trajectory, in keyframe coordinates, onto the
//                block's local knot parameters: dt_i = v - [t_i]x w, dw_i = R_i^T w
//   info_unit    (K P) A^T H_local A, H_local read as a symmetric unpack of the block's packed upper triangle
//   cov          sigma2 info_unit^-1 through a 6 x 6 Cholesky factorisation, one lane
//   flags        the chi test of detectOutliersAndUploadToGpu (blur_aware_direct_tracker.cpp:639-699) on the patch costs
//
// The statistic restates the one in k_lm_decide (lm_batch.hip) on purpose: that one is a wave of 64 lanes with the costs of small
// problems held in registers, this one a workgroup that strides over any K (grid picks: dozens; every candidate: up to H W), and
// sharing a body would change the LM's compiled code.  Both follow the same definition; their sums run in different orders, so
// their mu and bound agree to rounding, not to the bit.
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
        // the workgroup's sum of v in a fixed order -- butterfly within the wave, then the four waves in wave order -- in every lane
        __device__ __forceinline__ double block_sum(double v, double *s_w)
        {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
            __syncthreads(); // (the last sum has been read)
            if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
            __syncthreads();
            return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
        }

        template <int KDEG>
        __global__ __launch_bounds__(256) void k_pairs_report(const ReportArgs a)
        {
#pragma clang fp contract(off)
            constexpr int M = 6 * KDEG, ND = M + 1, E = ND * (ND + 1) / 2;
            __shared__ double s_H[M * M], s_A[M * 6], s_HA[M * 6], s_kt[3 * KDEG], s_kR[4 * KDEG], s_info[36], s_L[36], s_Li[36], s_T[7], s_w[4];
            __shared__ int s_before[4], s_idx;
            const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
            struct mbavo_pairs_report *out = a.out + b;
            const int K = a.counts[(size_t)b * a.L];
            // the evaluation packs the patch costs pair after pair: this pair's start at the sum of the K before it (integers: any order)
            int before = 0;
            for (int j = tid; j < b; j += 256) before += a.counts[(size_t)j * a.L];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) before += __shfl_xor(before, off);
            if (lane == 0) s_before[wave] = before;
            if (tid == 0)
            { // the pose at the capture time, as mbavo_pairs_assess samples it, and the segment it lies on
                const double cap = a.cap[b];
                int idx;
                double u, p[3];
                Quat q;
                const bool ok = spline_segment_checked(cap, a.t0[b], a.dt, a.N, KDEG, idx, u) && spline_pose<KDEG>(a.kt + (size_t)b * 3 * a.N, a.kR + (size_t)b * 4 * a.N, a.N, a.t0[b], a.dt, cap, q, p);
                s_idx = ok ? idx : -1;
                if (ok)
                {
                    s_T[0] = p[0]; s_T[1] = p[1]; s_T[2] = p[2];
                    s_T[3] = q.x; s_T[4] = q.y; s_T[5] = q.z; s_T[6] = q.w;
                }
            }
            __syncthreads();
            const int idx = s_idx;
            if (idx < 0)
            { // the capture time lies outside the knots
                if (tid == 0)
                {
                    const double nan = __builtin_nan("");
                    out->status = MBAVO_E_RANGE; out->num_keypoints0 = K; out->num_flagged = 0; out->num_stat = 0;
                    out->num_valid_px = nan; out->cost = nan; out->sigma2 = nan;
                    for (int i = 0; i < 7; ++i) out->T[i] = nan;
                    for (int i = 0; i < 36; ++i) { out->info_unit[i] = nan; out->cov[i] = nan; }
                }
                return;
            }
            const long long base = (long long)s_before[0] + s_before[1] + s_before[2] + s_before[3];
            const double *__restrict__ blk = a.blocks + (size_t)b * E;
            // H_local, both triangles, from the packed upper triangle behind [cost | g]: entry (r, c), r <= c, of the M x M triangle
            for (int t = tid; t < M * M; t += 256)
            {
                const int r = t / M, c = t - r * M, lo = r < c ? r : c, hi = r < c ? c : r;
                s_H[t] = blk[ND + lo * M - lo * (lo - 1) / 2 + (hi - lo)];
            }
            if (tid < 3 * KDEG) s_kt[tid] = a.kt[((size_t)b * a.N + idx) * 3 + tid];
            if (tid < 4 * KDEG) s_kR[tid] = a.kR[((size_t)b * a.N + idx) * 4 + tid];
            __syncthreads();
            if (tid < KDEG)
            { // knot i's six rows of A: [I | -[t_i]x] and [0 | R_i^T]
                const int i = tid;
                const double tx = s_kt[3 * i], ty = s_kt[3 * i + 1], tz = s_kt[3 * i + 2];
                const double qx = s_kR[4 * i], qy = s_kR[4 * i + 1], qz = s_kR[4 * i + 2], qw = s_kR[4 * i + 3];
                const double n = sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
                const double x = qx / n, y = qy / n, z = qz / n, w = qw / n;
                const double R[9] = {1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w),
                                     2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w),
                                     2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)};
                const double mtx[9] = {0.0, tz, -ty, -tz, 0.0, tx, ty, -tx, 0.0}; // -[t]x
#pragma unroll
                for (int r = 0; r < 3; ++r)
                {
                    double *rt = s_A + (3 * i + r) * 6, *rw = s_A + (3 * KDEG + 3 * i + r) * 6;
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                    {
                        rt[c] = r == c ? 1.0 : 0.0;
                        rt[3 + c] = mtx[3 * r + c];
                        rw[c] = 0.0;
                        rw[3 + c] = R[3 * c + r]; // (row r of R^T)
                    }
                }
            }
            __syncthreads();
            if (tid < M * 6)
            { // H A
                const int r = tid / 6, c = tid - r * 6;
                double acc = 0.0;
                for (int j = 0; j < M; ++j) acc += s_H[r * M + j] * s_A[j * 6 + c];
                s_HA[tid] = acc;
            }
            __syncthreads();
            const double KP = (double)K * (double)a.P;
            if (tid < 36)
            { // A^T (H A): the upper triangle, mirrored
                const int r = tid / 6, c = tid - r * 6;
                if (r <= c)
                {
                    double acc = 0.0;
                    for (int j = 0; j < M; ++j) acc += s_A[j * 6 + r] * s_HA[j * 6 + c];
                    const double v = KP * acc;
                    s_info[r * 6 + c] = v;
                    s_info[c * 6 + r] = v;
                }
            }
            // ---- the chi test on the patch costs (block_sum's barriers also publish s_info)
            const double *__restrict__ pc = a.patch_cost + base;
            double *pc_out = a.patch_cost_out ? a.patch_cost_out + (size_t)b * a.cap0 : nullptr;
            unsigned char *fl_out = a.flags_out ? a.flags_out + (size_t)b * a.cap0 : nullptr;
            double sum = 0.0, cnt = 0.0;
            for (int i = tid; i < K; i += 256)
            {
                const double c = pc[i];
                if (pc_out) pc_out[i] = c;
                if (c < 1e-8) continue;
                sum += c;
                cnt += 1.0;
            }
            sum = block_sum(sum, s_w);
            cnt = block_sum(cnt, s_w);
            const double mu = sum / cnt;
            double var = 0.0;
            for (int i = tid; i < K; i += 256)
            {
                const double c = pc[i];
                if (c < 1e-8) continue;
                var += (c - mu) * (c - mu);
            }
            var = block_sum(var, s_w) / cnt;
            const double bound = a.chi * (double)sqrtf((float)var);
            double nflag = 0.0;
            for (int i = tid; i < K; i += 256)
            {
                const bool f = cnt > 0.0 && fabs(pc[i] - mu) > bound;
                if (fl_out) fl_out[i] = f ? 1 : 0;
                if (f) nflag += 1.0;
            }
            nflag = block_sum(nflag, s_w);
            if (tid != 0) return;
            // ---- the record: one lane
            const double cost = blk[0], valid = a.valid[b];
            const double den = valid - 6.0 > 1.0 ? valid - 6.0 : 1.0;
            const double sigma2 = ((2.0 * cost) * KP) / den;
            bool ok = K > 0;
            for (int j = 0; j < 6 && ok; ++j)
            { // info_unit = L L^T
                double d = s_info[j * 6 + j];
                for (int k = 0; k < j; ++k) d -= s_L[j * 6 + k] * s_L[j * 6 + k];
                if (!(d > 0.0) || !(d < __builtin_inf())) { ok = false; break; }
                const double ljj = sqrt(d);
                s_L[j * 6 + j] = ljj;
                for (int i = j + 1; i < 6; ++i)
                {
                    double v = s_info[i * 6 + j];
                    for (int k = 0; k < j; ++k) v -= s_L[i * 6 + k] * s_L[j * 6 + k];
                    s_L[i * 6 + j] = v / ljj;
                }
            }
            if (ok)
            { // L^-1, column by column; cov = sigma2 L^-T L^-1, the upper triangle mirrored
                for (int c = 0; c < 6; ++c)
                {
                    s_Li[c * 6 + c] = 1.0 / s_L[c * 6 + c];
                    for (int i = c + 1; i < 6; ++i)
                    {
                        double v = 0.0;
                        for (int k = c; k < i; ++k) v += s_L[i * 6 + k] * s_Li[k * 6 + c];
                        s_Li[i * 6 + c] = -v / s_L[i * 6 + i];
                    }
                }
                for (int r = 0; r < 6; ++r)
                    for (int c = r; c < 6; ++c)
                    {
                        double v = 0.0;
                        for (int k = c; k < 6; ++k) v += s_Li[k * 6 + r] * s_Li[k * 6 + c];
                        out->cov[r * 6 + c] = sigma2 * v;
                        out->cov[c * 6 + r] = sigma2 * v;
                    }
            }
            else
                for (int i = 0; i < 36; ++i) out->cov[i] = __builtin_nan("");
            out->status = ok ? 0 : MBAVO_REPORT_SINGULAR;
            out->num_keypoints0 = K; out->num_flagged = (int)nflag; out->num_stat = (int)cnt;
            out->num_valid_px = valid; out->cost = cost; out->sigma2 = sigma2;
            for (int i = 0; i < 7; ++i) out->T[i] = s_T[i];
            for (int i = 0; i < 36; ++i) out->info_unit[i] = s_info[i];
        }

        // the launches of the evaluation the engine just enqueued, from its own witnesses (include/mbavo.h: mbavo_last_kernel,
        // mbavo_last_layout): the single-launch kernel, or pose kernel + fused kernel + finalize with the first two absent
        // where the fused kernel computes its own pose entries / where no pair has a tile
        long long evaluation_launches(Engine &eng)
        {
            int lay[8];
            eng.last_layout(lay);
            const char *name = eng.last_kernel();
            const size_t n = strlen(name);
            const bool last_true = n >= 6 && strcmp(name + n - 6, ",true>") == 0;
            if (strncmp(name, "k_fused_sp<", 11) == 0 && last_true) return 1;
            return (last_true ? 0 : 1) + (lay[0] > 0 ? 1 : 0) + 1;
        }
    } // namespace pairs

    using namespace pairs;

    int PairBatch::report(double chi, struct mbavo_pairs_report *h_out, double *d_patch_cost, unsigned char *d_flags)
    {
        if (!arena_ || !prepared_ || !motion_set_ || !h_out || !(chi >= 0) || !std::isfinite(chi)) return MBAVO_E_ARG;
        const PairsPlan &p = plan_;
        const int B = p.B, L = p.L, k = opts_.spline_deg_k, nd = 6 * k + 1, E = nd * (nd + 1) / 2;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        const size_t rec_bytes = sizeof(struct mbavo_pairs_report) * (size_t)B;
        const long long o_valid = align_up((long long)sizeof(double) * B * E, kAlign);
        const long long o_patch = o_valid + align_up((long long)sizeof(double) * B, kAlign);
        const long long o_rec = o_patch + align_up((long long)sizeof(double) * B * p.cap[0], kAlign);
        // the first report: its scratch (include/mbavo.h)
        if (!report_ && (e = report_.alloc((size_t)o_rec + rec_bytes)) != hipSuccess) return (int)e;
        if (!h_report_ && (e = h_report_.alloc(rec_bytes)) != hipSuccess) return (int)e;
        rep_stats_ = CallStats{};
        // the level-0 entries, one behind the other as the engine takes a list, with no keypoint excluded
        report_probs_.resize(B);
        for (int b = 0; b < B; ++b)
        {
            mbavo_problem &q = report_probs_[b];
            q = probs_[(size_t)b * L];
            q.d_outlier = nullptr; q.num_bad = 0; q.num_residuals = 0;
        }
        ReportArgs a;
        double *blocks = (double *)report_.p, *valid = (double *)(report_ + o_valid), *patch = (double *)(report_ + o_patch);
        int rc = eng_.evaluate(B, report_probs_.data(), k, true, blocks, patch, valid, nullptr);
        if (rc != 0) return rc;
        rep_stats_.launches = evaluation_launches(eng_);
        a.counts = lay_.counts(arena_);
        a.cap = lay_.cap(arena_); a.kt = lay_.knots_t(arena_); a.kR = lay_.knots_R(arena_);
        a.t0 = lay_.t0(arena_);
        a.blocks = blocks; a.patch_cost = patch; a.valid = valid;
        a.dt = probs_[0].dt; a.chi = chi;
        a.L = L; a.N = p.N; a.P = opts_.P[0]; a.cap0 = p.cap[0];
        a.out = (struct mbavo_pairs_report *)(report_ + o_rec);
        a.patch_cost_out = d_patch_cost; a.flags_out = d_flags;
        if (k == 2) hipLaunchKernelGGL(k_pairs_report<2>, dim3(B), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_pairs_report<4>, dim3(B), dim3(256), 0, st, a);
        ++rep_stats_.launches;
        return read_back(a.out, h_report_, h_out, rec_bytes, rep_stats_);
    }
} // namespace mbavo

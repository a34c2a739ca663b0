// pairs_track.hip -- the tracker of a batch of keyframe pairs (include/mbavo.h: mbavo_pairs_assess, _set_states, _get_states,
// _predict, _commit): what trackFrame does around the LM for one pair (blur_aware_direct_tracker.cpp:119-262), for B pairs with the
// pose state on the device, one launch per step whatever B is:
//
//   assess    isKeyframe, :205-262                 one workgroup per pair samples the pair's spline and sums the flow and the blur
//                                                  kernel of its level-0 keypoints
//   predict   :119-141                             the constant-velocity prediction moves every knot, 16 lanes per pair
//   commit    :143-203                             the assessment, then the pose bookkeeping of the frame and the re-expression
//                                                  of the knots for a new keyframe
//
// The images, gradients and keypoints these read are pairs_prep.hip's.  The two files share the device table (pairs_desc.h), the
// arena's layout (pairs_prep.h: PairsArena, the tracker's tail included), the end of a call that reads back (read_back) and two
// host helpers on the times of a frame, which set_motion and predict both need (samples_on_knots, publish_times: pairs_prep.hip).
#include "pairs_prep.h"
#include "pairs_desc.h"
#include "camera_math.h"
#include "pose_math.h"
#include "se3_math.h"
#include <cstring>
#include <hip/hip_runtime.h>

namespace mbavo
{
    namespace pairs
    {
        // ---- the keyframe test and the frame pose of every pair (vo_frontend.cpp: BlurAwareDirectTracker::isKeyframe,
        // blur_aware_direct_tracker.cpp:205-262): one workgroup per pair.  Lanes 0..2 sample the pair's spline at the capture time
        // and at -/+ half the exposure (SplineSE3::GetPose) and invert the poses (Core::Transformation::inverse) into LDS; every
        // lane then strides over the level-0 keypoints with the host loop's arithmetic, operation for operation (no contraction:
        // the host build has no FMA), and keeps two double sums.  The sums meet in a fixed order -- butterfly within the wave, then
        // the four waves in wave order -- so the result has the same bits whatever B is and wherever the workgroup ran.
        struct AssessArgs
        {
            const PairLevelDesc *desc;
            const int *counts;
            const double *cap, *exp, *kt, *kR, *t0;
            double dt, K[4], flow_mag0, flow_mag1, max_blur_kernel_mag;
            int L, N;
            mbavo_pairs_assessment *out;
            const PairCamera *cams; // PER_PAIR (mbavo_pairs_opts.num_cameras > 0): the level-0 intrinsics of every pair, in place of K
        };

        // pair b's assessment into *out, by the whole workgroup.  Returns -1 in every lane when one of the three times lies outside
        // the knots; else the verdict in lane 0 (0 in the others), and T = the pose at the capture time (shared memory, lane 0's
        // to read).  One body for k_pairs_assess and k_pairs_commit: the same operations, the same bits.  PER_PAIR: the intrinsics
        // are those of the pair's camera (one entry per workgroup, scalar loads); the arithmetic does not change.
        template <int KDEG, bool PER_PAIR>
        __device__ __forceinline__ int assess_pair(const AssessArgs &a, const int b, mbavo_pairs_assessment *out, const double *&T)
        {
            __shared__ double s_inv[3][7], s_T[7], s_sum[4][2];
            __shared__ int s_bad[3], s_behind[4];
            const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
            T = s_T;
            const int K = a.counts[(size_t)b * a.L]; // level 0 of the last prepare / update
            if (tid < 3)
            {
                const double cap = a.cap[b], ex = a.exp[b];
                const double t = tid == 0 ? cap : (tid == 1 ? cap - 0.5 * ex : cap + 0.5 * ex);
                Quat q;
                double p[3], T[7], Ti[7];
                const bool ok = spline_pose<KDEG>(a.kt + (size_t)b * 3 * a.N, a.kR + (size_t)b * 4 * a.N, a.N, a.t0[b], a.dt, t, q, p);
                s_bad[tid] = ok ? 0 : 1;
                if (ok)
                {
                    pose_make(q, p, T);
                    pose_inverse(T, Ti);
                    for (int i = 0; i < 7; ++i) s_inv[tid][i] = Ti[i];
                    if (tid == 0)
                    { // the pose as GetPose returns it
                        s_T[0] = p[0]; s_T[1] = p[1]; s_T[2] = p[2];
                        s_T[3] = q.x; s_T[4] = q.y; s_T[5] = q.z; s_T[6] = q.w;
                    }
                }
            }
            __syncthreads();
            if (s_bad[0] | s_bad[1] | s_bad[2])
            { // isKeyframe returns false before the loop
                if (tid == 0)
                {
                    const double nan = __builtin_nan("");
                    out->is_keyframe = 0; out->status = MBAVO_E_RANGE; out->num_keypoints0 = K; out->num_behind = 0;
                    out->avg_flow = nan; out->avg_kernel = nan;
                    for (int i = 0; i < 7; ++i) out->T[i] = nan;
                }
                return -1;
            }
            Quat qi[3];
            double ti[3][3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
            {
                ti[j][0] = s_inv[j][0]; ti[j][1] = s_inv[j][1]; ti[j][2] = s_inv[j][2];
                qi[j] = Quat{s_inv[j][3], s_inv[j][4], s_inv[j][5], s_inv[j][6]};
            }
            double fx = a.K[0], fy = a.K[1], cx = a.K[2], cy = a.K[3];
            if constexpr (PER_PAIR)
            {
                const PairCamera &pc = a.cams[b];
                fx = pc.fx; fy = pc.fy; cx = pc.cx; cy = pc.cy;
            }
            const PairLevelDesc &d = a.desc[(size_t)b * a.L];
            const double2 *__restrict__ kp_xy = reinterpret_cast<const double2 *>(d.kp_xy);
            const double *__restrict__ kp_z = d.kp_z;
            double flow = 0.0, kern = 0.0;
            int behind = 0;
            for (int i = tid; i < K; i += 256)
            {
#pragma clang fp contract(off)
                const double2 xy = kp_xy[i];
                const double x = xy.x, y = xy.y, z = kp_z[i];
                const double P[3] = {(x - cx) / fx * z, (y - cy) / fy * z, z};
                double pj[3][2] = {{0, 0}, {0, 0}, {0, 0}};
#pragma unroll
                for (int j = 0; j < 3; ++j)
                {
                    double Pc[3];
                    qrotate(qi[j], P, Pc);
                    Pc[0] += ti[j][0]; Pc[1] += ti[j][1]; Pc[2] += ti[j][2];
                    if (Pc[2] < 0) { ++behind; continue; }
                    pj[j][0] = fx * (Pc[0] / (Pc[2] + 1e-8)) + cx;
                    pj[j][1] = fy * (Pc[1] / (Pc[2] + 1e-8)) + cy;
                }
                flow += (pj[0][0] - x) * (pj[0][0] - x) + (pj[0][1] - y) * (pj[0][1] - y);
                kern += (pj[1][0] - pj[2][0]) * (pj[1][0] - pj[2][0]) + (pj[1][1] - pj[2][1]) * (pj[1][1] - pj[2][1]);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1)
            { // (a + b is commutative: every lane of the wave ends with the same bits)
                flow += __shfl_xor(flow, off);
                kern += __shfl_xor(kern, off);
                behind += __shfl_xor(behind, off);
            }
            if (lane == 0) { s_sum[wave][0] = flow; s_sum[wave][1] = kern; s_behind[wave] = behind; }
            __syncthreads();
            if (tid == 0)
            {
                const double sf = ((s_sum[0][0] + s_sum[1][0]) + s_sum[2][0]) + s_sum[3][0];
                const double sk = ((s_sum[0][1] + s_sum[1][1]) + s_sum[2][1]) + s_sum[3][1];
                const double avg_flow = sqrtf((float)(sf / K)), avg_kernel = sqrtf((float)(sk / K)); // (K = 0: NaN, every test below false)
                int kf = 0;
                if (avg_flow > a.flow_mag0 && avg_kernel < a.max_blur_kernel_mag) kf = 1;
                if (avg_flow > a.flow_mag1) kf = 1;
                out->is_keyframe = kf; out->status = 0; out->num_keypoints0 = K;
                out->num_behind = ((s_behind[0] + s_behind[1]) + s_behind[2]) + s_behind[3];
                out->avg_flow = avg_flow; out->avg_kernel = avg_kernel;
                for (int i = 0; i < 7; ++i) out->T[i] = s_T[i];
                return kf;
            }
            return 0;
        }
        template <int KDEG, bool PER_PAIR>
        __global__ __launch_bounds__(256) void k_pairs_assess(const AssessArgs a)
        {
            const double *T;
            (void)assess_pair<KDEG, PER_PAIR>(a, (int)blockIdx.x, a.out + blockIdx.x, T);
        }

        // ---- the tracker state of every pair (trackFrame's pose bookkeeping, blur_aware_direct_tracker.cpp:119-141 and 143-203),
        // kStateLen doubles per pair (pairs_desc.h)
        struct TrackArgs
        {
            double *state;                 // B x kStateLen
            double *kt, *kR;               // the knots the problems point at: B x 3N, B x 4N
            double *cap, *exp, *t0;        // the motion's times, B each: what the LM kernels and the assessment read
            const double *times;           // predict: [cap | exp | t0] as uploaded
            mbavo_pairs_frame *frames;     // commit: B
            int B, N;
        };

        // The constant-velocity prediction (:119-141): 16 lanes per pair, 16 pairs per workgroup.  The first lane of a pair forms
        // dT = exp(velocity * dt_frame) once, into LDS, keeps dt_frame for the commit and publishes the frame's times; lane i then
        // moves knot i: SplineSE3::TransformByRight.  A pair touches nothing of another's: the same bits for any B.
        __global__ __launch_bounds__(256) void k_pairs_predict(const TrackArgs p)
        {
            __shared__ double s_dT[16][7];
            const int g = threadIdx.x >> 4, i = threadIdx.x & 15, b = (int)blockIdx.x * 16 + g;
            if (b < p.B && i == 0)
            {
#pragma clang fp contract(off)
                double *st = p.state + (size_t)b * kStateLen;
                const double cap = p.times[b], ex = p.times[p.B + b], t0 = p.times[2 * p.B + b];
                const double dt_frame = cap - st[kStatePrevTime];
                double v[6], dT[7];
#pragma unroll
                for (int j = 0; j < 6; ++j) v[j] = st[kStateVelocity + j] * dt_frame;
                se3_exp(v, dT);
#pragma unroll
                for (int j = 0; j < 7; ++j) s_dT[g][j] = dT[j];
                st[kStateDtFrame] = dt_frame;
                p.cap[b] = cap; p.exp[b] = ex; p.t0[b] = t0;
            }
            __syncthreads();
            if (b < p.B && i < p.N)
            {
                double *kt = p.kt + ((size_t)b * p.N + i) * 3, *kR = p.kR + ((size_t)b * p.N + i) * 4;
                const double d[3] = {s_dT[g][0], s_dT[g][1], s_dT[g][2]};
                const Quat dq{s_dT[g][3], s_dT[g][4], s_dT[g][5], s_dT[g][6]}, R = load_quat(kR);
                double r[3];
                qrotate(R, d, r);
                kt[0] += r[0]; kt[1] += r[1]; kt[2] += r[2];
                const Quat n = qmul(R, dq);
                kR[0] = n.x; kR[1] = n.y; kR[2] = n.z; kR[3] = n.w;
            }
        }

        // The assessment and the state update behind it (:143-203), a workgroup per pair: assess_pair, then lane 0 does the pose
        // algebra of the frame (velocity, T_prev, and for a new keyframe T_keyframe and TransformTo's right factor), lanes 0 .. N-1
        // re-express their knot where the verdict is "keyframe", and lane 0 samples the knots as they now are for T_world.
        template <int KDEG, bool PER_PAIR>
        __global__ __launch_bounds__(256) void k_pairs_commit(const AssessArgs a, const TrackArgs c)
        {
            __shared__ double s_right[7], s_kt[16 * 3], s_kR[16 * 4];
            __shared__ int s_rebase;
            const int b = blockIdx.x, tid = threadIdx.x, N = c.N;
            mbavo_pairs_frame *f = c.frames + b;
            const double *T;
            const int verdict = assess_pair<KDEG, PER_PAIR>(a, b, &f->a, T);
            if (verdict < 0)
            { // the state stays as the predict left it
                if (tid == 0)
                    for (int i = 0; i < 7; ++i) f->T_world[i] = __builtin_nan("");
                return;
            }
            double Tk[7];
            if (tid == 0)
            {
#pragma clang fp contract(off)
                double *st = c.state + (size_t)b * kStateLen;
                double Tb[7], Tp[7], Tpi[7], dTn[7], lg[6];
                pose_make(Quat{T[3], T[4], T[5], T[6]}, T, Tb); // T_b2w
#pragma unroll
                for (int i = 0; i < 7; ++i) { Tk[i] = st[kStateKeyframe + i]; Tp[i] = st[kStatePrev + i]; }
                pose_inverse(Tp, Tpi);
                pose_mul(Tpi, Tb, dTn); // :150-155
                se3_log(dTn, lg);
                const double dt_frame = st[kStateDtFrame];
#pragma unroll
                for (int i = 0; i < 6; ++i) st[kStateVelocity + i] = lg[i] / dt_frame;
                int rebase = 0;
                if (verdict)
                { // :176-188
                    double Tn[7];
                    pose_mul(Tk, Tb, Tn);
#pragma unroll
                    for (int i = 0; i < 7; ++i) { Tk[i] = Tn[i]; st[kStateKeyframe + i] = Tn[i]; Tb[i] = i == 6 ? 1.0 : 0.0; }
                    // SplineSE3::TransformTo(cap, identity) (Spline.h:183-200): dR = R(cap)^-1, dt = R(cap)^-1 * (0 - t(cap))
                    const double n2 = T[3] * T[3] + T[4] * T[4] + T[5] * T[5] + T[6] * T[6];
                    if (n2 > 0)
                    {
                        const Quat qi{-T[3] / n2, -T[4] / n2, -T[5] / n2, T[6] / n2};
                        const Quat dR = qmul(qi, Quat{0.0, 0.0, 0.0, 1.0});
                        const double d[3] = {0.0 - T[0], 0.0 - T[1], 0.0 - T[2]};
                        double dt3[3];
                        qrotate(qi, d, dt3);
                        s_right[0] = dt3[0]; s_right[1] = dt3[1]; s_right[2] = dt3[2];
                        s_right[3] = dR.x; s_right[4] = dR.y; s_right[5] = dR.z; s_right[6] = dR.w;
                        rebase = 1;
                    }
                }
#pragma unroll
                for (int i = 0; i < 7; ++i) st[kStatePrev + i] = Tb[i];
                st[kStatePrevTime] = a.cap[b];
                s_rebase = rebase;
            }
            __syncthreads();
            if (tid < N)
            {
                double *kt = c.kt + ((size_t)b * N + tid) * 3, *kR = c.kR + ((size_t)b * N + tid) * 4;
                double t[3] = {kt[0], kt[1], kt[2]};
                Quat R = load_quat(kR);
                if (s_rebase)
                { // TransformByRight
                    const double d[3] = {s_right[0], s_right[1], s_right[2]};
                    double r[3];
                    qrotate(R, d, r);
                    t[0] += r[0]; t[1] += r[1]; t[2] += r[2];
                    R = qmul(R, Quat{s_right[3], s_right[4], s_right[5], s_right[6]});
                    kt[0] = t[0]; kt[1] = t[1]; kt[2] = t[2];
                    kR[0] = R.x; kR[1] = R.y; kR[2] = R.z; kR[3] = R.w;
                }
                s_kt[3 * tid] = t[0]; s_kt[3 * tid + 1] = t[1]; s_kt[3 * tid + 2] = t[2];
                s_kR[4 * tid] = R.x; s_kR[4 * tid + 1] = R.y; s_kR[4 * tid + 2] = R.z; s_kR[4 * tid + 3] = R.w;
            }
            __syncthreads();
            if (tid == 0)
            {
                Quat q;
                double p[3], P[7], Tw[7];
                if (spline_pose<KDEG>(s_kt, s_kR, N, a.t0[b], a.dt, a.cap[b], q, p))
                {
                    pose_make(q, p, P);
                    pose_mul(Tk, P, Tw);
                }
                else // (the same time on the same segment as above: cannot fail)
                    for (int i = 0; i < 7; ++i) Tw[i] = __builtin_nan("");
                for (int i = 0; i < 7; ++i) f->T_world[i] = Tw[i];
            }
        }
    } // namespace pairs

    using namespace pairs;

    AssessArgs PairBatch::assess_args(double flow_mag0, double flow_mag1, double max_blur_kernel_mag) const
    {
        AssessArgs a;
        a.desc = lay_.desc(arena_); a.counts = lay_.counts(arena_);
        a.cap = lay_.cap(arena_); a.exp = lay_.exp(arena_); a.kt = lay_.knots_t(arena_); a.kR = lay_.knots_R(arena_); a.t0 = lay_.t0(arena_);
        a.dt = probs_[0].dt;
        for (int i = 0; i < 4; ++i) a.K[i] = opts_.intrinsics[i];
        a.cams = opts_.num_cameras > 0 ? lay_.pair_cameras(arena_) : nullptr;
        a.flow_mag0 = flow_mag0; a.flow_mag1 = flow_mag1; a.max_blur_kernel_mag = max_blur_kernel_mag;
        a.L = plan_.L; a.N = plan_.N;
        a.out = (mbavo_pairs_assessment *)step_.p;
        return a;
    }

    TrackArgs PairBatch::track_args() const
    {
        TrackArgs t;
        t.state = lay_.state(arena_); t.times = lay_.times(arena_); t.frames = lay_.frames(arena_);
        t.cap = lay_.cap(arena_); t.exp = lay_.exp(arena_); t.kt = lay_.knots_t(arena_); t.kR = lay_.knots_R(arena_); t.t0 = lay_.t0(arena_);
        t.B = plan_.B; t.N = plan_.N;
        return t;
    }

    // [knots_t | knots_R | pad | t0 | state]: what set_states uploads and get_states reads back, in one copy (PairsArena's span)
    int PairBatch::set_states(const mbavo_vo_state *h)
    {
        if (!arena_ || !h) return MBAVO_E_ARG;
        const int B = plan_.B, L = plan_.L, N = plan_.N;
        for (int b = 0; b < B; ++b)
            if (h[b].N != N || h[b].is_first != 0 || !(h[b].dt > 0) || h[b].dt != h[0].dt) return MBAVO_E_ARG;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        const long long first = lay_.span_first;
        double *kt = lay_.knots_t(h_state_, first), *kR = lay_.knots_R(h_state_, first);
        double *t0 = lay_.t0(h_state_, first), *sv = lay_.state(h_state_, first);
        for (int b = 0; b < B; ++b)
        {
            memcpy(kt + (size_t)b * 3 * N, h[b].knots_t, sizeof(double) * 3 * N);
            memcpy(kR + (size_t)b * 4 * N, h[b].knots_R, sizeof(double) * 4 * N);
            t0[b] = h[b].t0;
            double *v = sv + (size_t)b * kStateLen;
            memcpy(v + kStateKeyframe, h[b].T_keyframe, sizeof(double) * 7);
            memcpy(v + kStatePrev, h[b].T_prev_b2w, sizeof(double) * 7);
            memcpy(v + kStateVelocity, h[b].velocity, sizeof(double) * 6);
            v[kStatePrevTime] = h[b].prev_timestamp;
            v[kStateDtFrame] = 0.0;
        }
        hipStream_t st = eng_.stream();
        if ((e = hipMemcpyAsync(lay_.knots_t(arena_), h_state_, (size_t)lay_.span_bytes, hipMemcpyHostToDevice, st)) != hipSuccess) return (int)e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return (int)e; // (the staging buffer is free again)
        state_dt_ = h[0].dt;
        for (int i = 0; i < B * L; ++i) probs_[i].dt = state_dt_;
        for (int b = 0; b < B; ++b)
            for (int l = 0; l < L; ++l) probs_[(size_t)b * L + l].t0 = h[b].t0;
        states_set_ = true;
        pending_ = false;
        return 0;
    }

    int PairBatch::get_states(mbavo_vo_state *h)
    {
        if (!arena_ || !h || !states_set_) return MBAVO_E_ARG;
        const int B = plan_.B, N = plan_.N;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        const long long first = lay_.span_first;
        hipStream_t st = eng_.stream();
        if ((e = hipMemcpyAsync(h_state_, lay_.knots_t(arena_), (size_t)lay_.span_bytes, hipMemcpyDeviceToHost, st)) != hipSuccess) return (int)e;
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return (int)e;
        const double *kt = lay_.knots_t(h_state_, first), *kR = lay_.knots_R(h_state_, first);
        const double *t0 = lay_.t0(h_state_, first), *sv = lay_.state(h_state_, first);
        for (int b = 0; b < B; ++b)
        {
            memset(&h[b], 0, sizeof(h[b]));
            h[b].t0 = t0[b]; h[b].dt = state_dt_; h[b].N = N; h[b].is_first = 0;
            memcpy(h[b].knots_t, kt + (size_t)b * 3 * N, sizeof(double) * 3 * N);
            memcpy(h[b].knots_R, kR + (size_t)b * 4 * N, sizeof(double) * 4 * N);
            const double *v = sv + (size_t)b * kStateLen;
            memcpy(h[b].T_keyframe, v + kStateKeyframe, sizeof(double) * 7);
            memcpy(h[b].T_prev_b2w, v + kStatePrev, sizeof(double) * 7);
            memcpy(h[b].velocity, v + kStateVelocity, sizeof(double) * 6);
            h[b].prev_timestamp = v[kStatePrevTime];
        }
        return 0;
    }

    // (h_times_ is free: the last copy out of it was followed by a commit, a set_states or a call that synchronised itself)
    hipError_t PairBatch::upload_times(const double *h_cap, const double *h_exp)
    {
        const int B = plan_.B;
        for (int b = 0; b < B; ++b) { h_times_[b] = h_cap[b]; h_times_[B + b] = h_exp[b]; h_times_[2 * B + b] = h_cap[b] - 0.5 * h_exp[b]; }
        return hipMemcpyAsync(lay_.times(arena_), h_times_, sizeof(double) * 3 * B, hipMemcpyHostToDevice, eng_.stream());
    }

    int PairBatch::predict(const double *h_cap, const double *h_exp)
    {
        if (!arena_ || !prepared_ || !states_set_ || pending_ || !h_cap || !h_exp) return MBAVO_E_ARG;
        const int B = plan_.B;
        const double dt = state_dt_;
        // the host does the time arithmetic only, as set_motion does: nothing is touched before every pair has passed
        if (!samples_on_knots(h_cap, h_exp, nullptr, dt)) return MBAVO_E_RANGE;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        pre_stats_ = CallStats{};
        if ((e = upload_times(h_cap, h_exp)) != hipSuccess) return (int)e;
        const TrackArgs t = track_args();
        hipLaunchKernelGGL(k_pairs_predict, dim3((B + 15) / 16), dim3(256), 0, st, t);
        pre_stats_.launches = 1;
        if ((e = hipGetLastError()) != hipSuccess) return (int)e;
        publish_times(h_cap, h_times_ + 2 * B, dt);
        motion_set_ = true; // (times and knots are all there for mbavo_pairs_assess too)
        pending_ = true;
        return 0;
    }

    int PairBatch::commit(double flow_mag0, double flow_mag1, double max_blur_kernel_mag, mbavo_pairs_frame *h_out)
    {
        if (!arena_ || !pending_ || !h_out) return MBAVO_E_ARG;
        const int B = plan_.B;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        com_stats_ = CallStats{};
        AssessArgs a = assess_args(flow_mag0, flow_mag1, max_blur_kernel_mag);
        a.out = nullptr; // (the assessment goes into the frame record)
        const TrackArgs t = track_args();
        const bool per_pair = opts_.num_cameras > 0;
        if (opts_.spline_deg_k == 2) hipLaunchKernelGGL((per_pair ? k_pairs_commit<2, true> : k_pairs_commit<2, false>), dim3(B), dim3(256), 0, st, a, t);
        else hipLaunchKernelGGL((per_pair ? k_pairs_commit<4, true> : k_pairs_commit<4, false>), dim3(B), dim3(256), 0, st, a, t);
        com_stats_.launches = 1;
        pending_ = false; // (the state has moved on, whatever the launch and the copy say)
        return read_back(t.frames, h_frames_, h_out, sizeof(mbavo_pairs_frame) * B, com_stats_);
    }

    int PairBatch::assess(double flow_mag0, double flow_mag1, double max_blur_kernel_mag, mbavo_pairs_assessment *h_out)
    {
        if (!arena_ || !prepared_ || !motion_set_ || !h_out) return MBAVO_E_ARG;
        const int B = plan_.B;
        hipError_t e = hipSetDevice(eng_.device());
        if (e != hipSuccess) return (int)e;
        hipStream_t st = eng_.stream();
        ass_stats_ = CallStats{};
        const AssessArgs a = assess_args(flow_mag0, flow_mag1, max_blur_kernel_mag);
        const bool per_pair = opts_.num_cameras > 0;
        if (opts_.spline_deg_k == 2) hipLaunchKernelGGL((per_pair ? k_pairs_assess<2, true> : k_pairs_assess<2, false>), dim3(B), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((per_pair ? k_pairs_assess<4, true> : k_pairs_assess<4, false>), dim3(B), dim3(256), 0, st, a);
        ass_stats_.launches = 1;
        return read_back(a.out, h_assess_, h_out, sizeof(mbavo_pairs_assessment) * B, ass_stats_);
    }
} // namespace mbavo

// lm_batch.hip -- device-side Levenberg-Marquardt over a batch of independent alignment problems
// (SURVEY.md 8f row 4): what BlurAwareDirectTracker::optimizePyramidLevel does for ONE problem with a host round trip
// per evaluation (ba_tracker/blur_aware_direct_tracker.cpp:590-924) runs here for B problems with no host
// involvement inside an iteration: the packed blocks never leave the device, the 6N x 6N systems are assembled,
// damped and solved by one wave per problem, the accept / reject decision, the LM radius, the non-monotonic
// step evaluator and the outlier statistics are per-problem device state.  With a host loop the solve of 512
// systems (10 ms on one core) dwarfs the 0.16 ms evaluation; here an iteration is eight launches.
//
//   merge                ba_tracker/merge_hessian_gradient_cost.cpp:39-86
//   solve                ba_tracker/solve_normal_equation.h:10-35 (one-sided Jacobi SVD / pivoted LDL^T, the same
//                        algorithms as host_math.cpp, rows spread over the lanes of a wave)
//   LM radius            ba_tracker/levenberg_marquardt_strategy.cpp:9-45
//   step evaluator       ba_tracker/trust_region_step_evaluator.cpp:45-126
//   loop / outliers      ba_tracker/blur_aware_direct_tracker.cpp:590-699,799-924 (see tracker.cpp for the quirks kept)
//
// Per iteration slot:  k_lm_solve -> cost-only pass on the candidates -> k_lm_decide -> H/g pass on the accepted.
// Problems that are finished, took an invalid step or rejected their step sit the passes out (ProblemDesc::active).
#include "../../include/mbavo.h"
#include "engine.h"
#include "pixel_math.h"
#include "se3_math.h"
// The one-wave solvers of lm_solvers.h (one-sided Jacobi SVD, pivoted LDL^T) synchronise their steps with MBAVO_SOLVER_SYNC: a
// wave-level fence here -- LDS executes a wave's operations in order, so that is all a wave working alone needs, in the one-wave
// workgroups (k_lm_solve<KD, 64>) and as wave 0 of the wide ones (k_lm_solve<KD, kEigT> with solver type 1).
#define MBAVO_SOLVER_SYNC()                                   \
    do                                                        \
    {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                      \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
    } while (0)
#include "lm_solvers.h"
#include "lm_state.h"
#include "host_math.h"
#include "lm_batch.h"
#include "pose_entries.h"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <vector>

namespace mbavo
{
    // Where the sums of a (problem, frame) slot come from: the frame blocks a finalize kernel wrote, or -- deferred
    // (engine.h: set_defer_finalize) -- the tile partials themselves, added in k_finalize_flat's order ((t0 + t2) + (t1 + t3),
    // absent tiles = +0) and scaled by the same residual scale: the same bits, two launches fewer per LM iteration.
    struct FinSrc
    {
        const double *fb;        // frame blocks (E doubles per slot: [cost | g | H packed])
        const double *partials;  // deferred: tile partials, `stride` doubles each: [valid | g, H sums | cost | spare]
        const int *tile_begin;   // deferred: slot bf owns tiles [tile_begin[bf], tile_begin[bf + 1])
        int stride, deferred;
        int f1;                  // every problem has ONE frame: slot == problem index, so the slot's tile range, start index and residual
                                 // scale can be fetched at kernel entry, beside the descriptor instead of behind it (round 5: the merge
                                 // was a chain descriptor -> tile range -> partials of three memory latencies)
        const double *inv;       // f1: the residual scales, [problem]
    };
    __device__ __forceinline__ double slot_sum_range(const FinSrc &fs, int t0, int n, int e)
    {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n) t[i] = fs.partials[(size_t)(t0 + i) * fs.stride + e];
        return (t[0] + t[2]) + (t[1] + t[3]);
    }
    __device__ __forceinline__ double slot_sum(const FinSrc &fs, int bf, int e)
    {
        const int t0 = fs.tile_begin[bf];
        return slot_sum_range(fs, t0, fs.tile_begin[bf + 1] - t0, e);
    }
    template <int E>
    __device__ __forceinline__ double slot_cost(const FinSrc &fs, int bf)
    {
        return fs.deferred ? slot_sum(fs, bf, E) : fs.fb[(size_t)bf * E]; // (patch costs are scaled when they are computed)
    }

    // The host's view of the loop without a copy or an event in the stream: the last workgroup of a k_lm_solve launch stores
    // (slot + 1) << 32 | problems done into a pinned host word.
    // Ticket and done count are ONE 64-bit word (num_done[6..7]; low half: workgroups that have passed, over all launches of the
    // call; high half: problems done), bumped by one atomic -- the workgroup whose ticket completes (slot + 1) B sees every other
    // workgroup's contribution in the value the atomic returns: no fence, no second counter read.
    // (round 4) The completing workgroup also leaves the engine's range-status counter in pinned memory (host_word[4], as an int)
    // before the word: with every problem's final state stored to pinned memory by the workgroup that ended it (k_lm_solve), a
    // finished call needs no copy back and no blocking stream synchronisation (~20 us of a 64-pair call).
    __device__ __forceinline__ void slot_publish(int *num_done, unsigned long long *host_word, int slot, int B, bool done_now,
                                                 const int *status_src = nullptr)
    {
        if (!host_word) return;
        unsigned long long *ticket = reinterpret_cast<unsigned long long *>(num_done + 6);
        const unsigned long long old = atomicAdd(ticket, 1ull + (done_now ? 1ull << 32 : 0ull));
        if ((unsigned)(old & 0xffffffffull) + 1u != (unsigned)(slot + 1) * (unsigned)B) return;
        // The completing workgroup: every other workgroup made its stores (final states in pinned memory, the status counter)
        // visible with a system-scope fence BEFORE its relaxed ticket; this acquire fence after the ticket that read theirs
        // pairs with those fences (fence-to-fence synchronisation), so the release store of the word below publishes all of
        // them -- by the memory model, not only by how gfx9 drains a system fence.
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const unsigned nd = (unsigned)(old >> 32) + (done_now ? 1u : 0u);
        if (status_src != nullptr)
            __hip_atomic_store(reinterpret_cast<int *>(host_word + 4), __hip_atomic_load(status_src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(host_word, ((unsigned long long)(slot + 1) << 32) | nd, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // The same for the decide launch of a slot, with the LOOK-AHEAD count (round 4): how many problems the NEXT solve launch will
    // find finished (already done, or its loop check `iter + 1 > max_it || abs_dec < min_dec` will end them).  When that is all B,
    // the host -- which has the next solve queued and reads this word before it enqueues that slot's three passes -- enqueues
    // none: no idle launches behind the last solve (4 x ~4.6 us per call before).  Ticket word: num_done[8..9], the low half
    // counts workgroups over all decide launches of the call, the high half is reset by the completing workgroup.
    __device__ __forceinline__ void decide_publish(int *num_done, unsigned long long *host_word2, int slot, int B, bool will_finish)
    {
        if (!host_word2) return;
        unsigned long long *ticket = reinterpret_cast<unsigned long long *>(num_done + 8);
        const unsigned long long old = atomicAdd(ticket, 1ull + (will_finish ? 1ull << 32 : 0ull));
        if ((unsigned)(old & 0xffffffffull) + 1u != (unsigned)(slot + 1) * (unsigned)B) return;
        const unsigned nf = (unsigned)(old >> 32) + (will_finish ? 1u : 0u);
        atomicAdd(ticket, 0ull - ((unsigned long long)nf << 32)); // the count starts over for the next slot's decide launch
        __hip_atomic_store(host_word2, ((unsigned long long)(slot + 1) << 32) | nf, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __device__ __forceinline__ bool lm_will_finish(const LmState &s, const LmOpts &o)
    { // k_lm_solve's loop check, one launch ahead; the end of a coarser level is a level switch, not a finish
        return s.done != 0 || ((s.iter + 1 > o.max_it || s.abs_dec < o.min_dec) && s.level == 0);
    }

    // One workgroup of T threads per problem (per PAIR with levels: o.levels > 1, see lm_batch): finish the previous accepted step,
    // loop control, damping, solve, model change, candidate.  T = 64 (one wave: the one-sided Jacobi SVD / pivoted LDL^T of lm_solvers.h, any n up to 96) or T = kEigT
    // (solver 0 with n <= kEigMaxN: the workgroup-parallel eigenvalue Jacobi, eig_solve).  The scalar state of the loop is
    // computed redundantly by every thread (same inputs, same arithmetic); thread 0 stores it.
    template <int KD, int T>
    __global__ __launch_bounds__(T) void k_lm_solve(const ProblemDesc *__restrict__ descs, LmState *__restrict__ states, LmOpts o,
                                                    FinSrc fs, const int *__restrict__ start_idx,
                                                    double *__restrict__ Hst, double *__restrict__ gst,
                                                    double *__restrict__ cur_t, double *__restrict__ cur_R,
                                                    int *__restrict__ active, mbavo_trace_rec *__restrict__ trace,
                                                    int *__restrict__ num_done, unsigned long long *host_word, int slot, int B,
                                                    PoseEntry<KD> *pose_table, int *pose_status, LmState *h_final)
    {
        constexpr int M6 = 6 * KD, ND = M6 + 1, E = ND * (ND + 1) / 2;
        extern __shared__ __attribute__((aligned(16))) double lds[];
        const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
        // the engine's entry of the pair: b itself, or -- levels -- b * levels + the pair's current level (one load more)
        const int e = o.levels > 1 ? b * o.levels + states[b].level : b;
        const ProblemDesc &d = descs[e];
        // one-frame batches: the first slot's tile range, start index and scale do not wait for the descriptor
        int e_t0 = 0, e_t1 = 0, e_st0 = 0;
        double e_inv = 0.0;
        if (fs.f1 && fs.deferred)
        {
            e_t0 = fs.tile_begin[e]; e_t1 = fs.tile_begin[e + 1]; e_st0 = start_idx[e];
            e_inv = fs.inv[e];
        }
        const int N = d.N, n = 6 * N, F = d.F;
        LmState s = states[b]; // (slot 0: the initial state, uploaded by the host with the head of the arena)
        if (s.done)
        {
            if (tid == 0) slot_publish(num_done, host_word, slot, B, false, pose_status);
            return;
        }
        if (slot == 0)
        { // the current point starts at the caller's knots (there is no init launch: one kernel less in every call)
            double *Ct0 = cur_t + (size_t)b * 3 * o.max_N, *CR0 = cur_R + (size_t)b * 4 * o.max_N;
            for (int i = tid; i < 3 * N; i += T) Ct0[i] = d.knots_t[i];
            for (int i = tid; i < 4 * N; i += T) CR0[i] = d.knots_R[i];
            __syncthreads();
        }
#if defined(MBAVO_EIG_STAMPS) // development aid: where the kernel's time goes (block 0 prints at its end)
        const long long ts0 = __builtin_amdgcn_s_memtime();
        long long ts1 = 0, ts2 = 0, ts3 = 0;
#endif
        // LDS, T = 64: V and G (n x (n + 1) each) + vectors; the damped system H itself lives in global memory (it persists
        // across iterations anyway), which leaves room for the reference's maximum of 16 control knots (n = 96).
        // T = kEigT: the four n x eig_ld(n) areas of eig_solve first (16-byte aligned), then the vectors.
        // T = kEigT additionally keeps the system itself in LDS for the length of the kernel (merge, damping, model change:
        // ~25 dependent global round trips otherwise); global memory holds it between launches.
        constexpr bool eig = T == kEigT; // the host launches this form when every n <= kEigMaxN
        double *V = lds, *g = V + (eig ? eig_lds_doubles(n) : (size_t)n * (n + 1)), *x = g + n, *tmp = x + n;
        double *Hl = tmp + n;                                        // T = kEigT: n x n
        int *order = eig ? (int *)(Hl + n * n) : (int *)(tmp + n);   // T = kEigT: eig_solve's 4 + 2 n ints
        double *Hg = Hst + (size_t)b * o.max_n * o.max_n, *gg = gst + (size_t)b * o.max_n;
        double *H = eig ? Hl : Hg;
        double *Ct = cur_t + (size_t)b * 3 * o.max_N, *CR = cur_R + (size_t)b * 4 * o.max_N;
        mbavo_trace_rec *tr = trace ? trace + (size_t)b * o.trace_cap : nullptr;

        if (s.fresh)
        { // the H/g pass at the current point has completed: its cost is the evaluation-point cost
            // Frame 0's packed entries (1 .. E - 1: g, then the upper triangle of H) for this thread are FETCHED FIRST, together with the
            // costs, and scattered after the bookkeeping: one memory latency for all of it instead of a dependent chain cost ->
            // bookkeeping -> g -> H (the kernel is a chain of such round trips: 11 700 of its 37 000 cycles were this merge).
            constexpr int kEntries = E - 1, kPer = (kEntries + T - 1) / T;
            const bool early = fs.f1 && fs.deferred;
            const double inv = early ? e_inv : (fs.deferred ? (d.inv_ptr != nullptr ? *d.inv_ptr : d.inv_num_residuals) : 0.0);
            const int bf0 = early ? e : d.bf_base, st0 = early ? e_st0 : start_idx[bf0];
            double val[kPer];
#pragma unroll
            for (int q = 0; q < kPer; ++q)
            {
                const int p = 1 + tid + q * T;
                val[q] = p <= kEntries ? (early ? slot_sum_range(fs, e_t0, e_t1 - e_t0, p) * inv
                                                : (fs.deferred ? slot_sum(fs, bf0, p) * inv : fs.fb[(size_t)bf0 * E + p])) : 0.0;
            }
            double cost = 0.0;
            if (early) cost = slot_sum_range(fs, e_t0, e_t1 - e_t0, E);
            else
                for (int f = 0; f < F; ++f) cost += slot_cost<E>(fs, d.bf_base + f);
            s.eval_cost = cost;
            if (s.pending_accept)
            { // handleSuccessfulStep (:896-903)
                lm_accepted(s, s.quality);
                tr_accepted(s, s.eval_cost, s.model, o.max_nonmono);
                trace_push(s, tr, o.trace_cap, tid, s.level, 1, s.cand_cost, s.model, s.quality);
                ++s.n_accept;
            }
            else
            { // iteration 0 of the level (:590-606); the call's initial cost is the coarsest level's
                if (s.level == o.levels - 1) s.initial_cost = cost;
                lm_reset(s);
                tr_reset(s, cost);
                trace_push(s, tr, o.trace_cap, tid, s.level, 0, 0.0, 0.0, 0.0);
            }
            // merge_hessian_gradient_cost.cpp:39-86, frames in order
            for (int i = tid; i < n * n; i += T) H[i] = 0.0;
            for (int i = tid; i < n; i += T) g[i] = 0.0;
            __syncthreads();
            auto knot_row = [&](int j, int st) { return j < 3 * KD ? 3 * st + j : 3 * (N + st) + (j - 3 * KD); };
#pragma unroll
            for (int q = 0; q < kPer; ++q)
            { // frame 0, from the registers (distinct entries per thread: no two threads add into the same word)
                const int p = 1 + tid + q * T;
                if (p <= M6)
                    g[knot_row(p - 1, st0)] += val[q];
                else if (p <= kEntries)
                {
                    int r, c;
                    tri_decode(p - ND, M6, r, c);
                    const int R = knot_row(r, st0), C = knot_row(c, st0);
                    H[C * n + R] += val[q];
                    if (R != C) H[R * n + C] += val[q];
                }
            }
            __syncthreads();
            for (int f = 1; f < F; ++f)
            {
                const int bf = d.bf_base + f;
                const double *blk = fs.fb + (size_t)bf * E;
                const int st = start_idx[bf];
                for (int j = tid; j < M6; j += T) g[knot_row(j, st)] += fs.deferred ? slot_sum(fs, bf, 1 + j) * inv : blk[1 + j];
                for (int e = tid; e < M6 * (M6 + 1) / 2; e += T)
                {
                    int r, c;
                    tri_decode(e, M6, r, c);
                    const int R = knot_row(r, st), C = knot_row(c, st);
                    const double v = fs.deferred ? slot_sum(fs, bf, ND + e) * inv : blk[ND + e];
                    H[C * n + R] += v;
                    if (R != C) H[R * n + C] += v;
                }
                __syncthreads();
            }
            for (int i = tid; i < n; i += T) gg[i] = g[i];
            s.fresh = 0;
            s.pending_accept = 0;
        }
        else
        {
            for (int i = tid; i < n; i += T) g[i] = gg[i];
            if (eig)
                for (int i = tid; i < n * n; i += T) Hl[i] = Hg[i];
        }
        __syncthreads();

        // finalizeIterationAndCheckIfMinimizerCanContinue (:910-924)
        ++s.iter;
        if (s.iter > o.max_it || s.abs_dec < o.min_dec)
        {
            --s.iter;
            if (s.level > 0)
            { // the end of a coarser pyramid level (optimizeTrajectory, :571-575): the pair goes on to the next finer one at once --
              // it waits for no other pair.  Its accepted point (the level's last candidate may be in the shared knot buffers) is
              // where the new level starts; optimizePyramidLevel's fresh start (:590-606) follows: this slot's H/g pass evaluates the
              // new entry (active 2), the next launch merges that as iteration 0 and resets the LM radius and the step evaluator.
                // The flags of the new entry are its own, still clear (zeroed with the head); so is its residual scale.
                double *Wt = const_cast<double *>(d.knots_t), *WR = const_cast<double *>(d.knots_R);
                for (int i = tid; i < 3 * N; i += T) Wt[i] = Ct[i];
                for (int i = tid; i < 4 * N; i += T) WR[i] = CR[i];
                s.iter_sum += s.iter;
                --s.level;
                s.iter = 0; s.abs_dec = 1e10; s.num_bad = 0;
                s.eval_cost = 0.0; s.cand_cost = 0.0; s.model = 0.0; s.quality = 0.0;
                s.fresh = 1; s.pending_accept = 0; s.done = 0;
                if (tid == 0)
                {
                    active[e] = 0;
                    active[e - 1] = 2;
                    states[b] = s;
                    slot_publish(num_done, host_word, slot, B, false, pose_status);
                }
                // the passes read the pose entries from the table (Engine::set_external_poses): the new entry's, at the current
                // point, with the knot Jacobians -- as for a candidate below
                if constexpr (T >= 64 * KD)
                {
                    if (pose_table != nullptr)
                    {
                        const ProblemDesc &dn = descs[e - 1];
                        double *Lt = V, *LR = V + 3 * N;
                        for (int i = tid; i < 3 * N; i += T) Lt[i] = Ct[i];
                        for (int i = tid; i < 4 * N; i += T) LR[i] = CR[i];
                        __syncthreads();
                        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
                        SplineSeg *segs = (SplineSeg *)(V + 8 * N);
                        for (int f = 0; f < F; ++f)
                        {
                            frame_pose_entries<KD, true>(dn, Lt, LR, f, pose_table + dn.pose_base + f * dn.S, segs, wave, lane, pose_status, true);
                            __syncthreads();
                        }
                    }
                }
                return;
            }
            s.done = 1;
            if (tid == 0)
            {
                active[e] = 0;
                states[b] = s;
                if (h_final != nullptr)
                { // the final state straight into pinned host memory, on its way before this workgroup counts as passed
                    h_final[b] = s;
                    __threadfence_system();
                }
                atomicAdd(num_done, 1); // (what the stream-drain scheme and the final check read)
                slot_publish(num_done, host_word, slot, B, true, pose_status);
            }
            // leave the accepted point in the caller's knot buffers
            double *Wt = const_cast<double *>(d.knots_t), *WR = const_cast<double *>(d.knots_R);
            for (int i = tid; i < 3 * N; i += T) Wt[i] = Ct[i];
            for (int i = tid; i < 4 * N; i += T) WR[i] = CR[i];
            return;
        }

#if defined(MBAVO_EIG_STAMPS)
        ts1 = __builtin_amdgcn_s_memtime();
#endif
        // computeTrustRegionStep (:799-831): the damping is applied in place and accumulates over rejected steps
        const double iradius = 1. / s.radius;
        for (int i = tid; i < n; i += T)
        {
            const double v = H[i * n + i] + H[i * n + i] * iradius;
            H[i * n + i] = v;
        }
        __syncthreads();
        if (eig)
            for (int i = tid; i < n * n; i += T) Hg[i] = Hl[i]; // the damped system, for the next launch
        // the solvers destroy their matrix: work on a copy in V's place (LDLT, eigenvalue Jacobi) or keep H in V and rotate a
        // copy (one-sided SVD)
#if defined(MBAVO_EIG_STAMPS)
        ts2 = __builtin_amdgcn_s_memtime();
#endif
        // LDL^T in registers (wave 0) stands in for the Jacobi SVD (solver 0) or the pivoted LDL^T (solver 1) when every pivot is positive and the pivot ratio is
        // at most fast_ratio -- the host loop's rule (host_math.cpp:solve_spd_fast, MBAVO_FAST_SOLVE) -- and, refined in
        // double-double, up to refined_ratio when the refinement converges (lm_solvers.h: spd_solve_regs_impl; MBAVO_LM_REFINE=0
        // switches that off); any other system takes the solver below.  11 000 cycles (22 000 refined) against 138 000 for
        // the eigenvalue Jacobi or the pivoted LDL^T at n = 24 (tests/harness/solver_check.hip), and a launch lasts as long as
        // its slowest system: before the refined form, one system of 64 above the ratio held every launch for 75 us.
        bool have = false;
        if (o.fast_ratio > 0.0 && (n == 12 || n == 18 || n == 24)) // (solver 1 too: its pivoted LDL^T walks 2 000 cycles per column)
        {
            if (tid < 64)
            {
                bool ok;
                if (n == 12) ok = spd_solve_regs_impl<12, true>(H, g, x, lane, o.fast_ratio, o.refined_ratio);
                else if (n == 18) ok = spd_solve_regs_impl<18, true>(H, g, x, lane, o.fast_ratio, o.refined_ratio);
                else ok = spd_solve_regs_impl<24, true>(H, g, x, lane, o.fast_ratio, o.refined_ratio);
                if (tid == 0) order[0] = ok ? 1 : 0;
            }
            __syncthreads();
            have = order[0] != 0;
            __syncthreads(); // `order` is the Jacobi solvers' work area
            if (have && tid == 0) atomicAdd(num_done + 5, 1);
        }
        else if (o.fast_ratio > 0.0 && n <= 64)
        { // 5 .. 10 control knots: the same factorisation by the whole workgroup in LDS (V's place), the system read where it lives
            have = spd_solve_coop<T>(V, H, g, x, tmp, order, n, tid, o.fast_ratio, o.refined_ratio);
            if (have && tid == 0) atomicAdd(num_done + 5, 1);
        }
        if (have) {}
        else if constexpr (T == kEigT)
        {
          if (o.solver == 1)
          { // the reference's LDLT option in the wide workgroup (round 4: so that its candidates get their pose entries here too):
            // the pivoted LDL^T of lm_solvers.h by wave 0 on a copy, the other waves wait
            for (int i = tid; i < n * n; i += T) V[i] = H[i];
            __syncthreads();
            if (tid < 64) ldlt_solve(V, g, x, tmp, order, n, lane);
            __syncthreads();
          }
          else
          {
            const int info = eig_solve(V, Hl, g, x, tmp, order, n, tid);
            if (tid == 0)
            { // solver statistics in the spare words behind num_done (MBAVO_LM_STATS=1 prints them)
                atomicAdd(num_done + 1, 1);
                atomicAdd(num_done + 2, info & 255);
                atomicMax(num_done + 3, info & 255);
                atomicAdd(num_done + 4, info >> 8);
            }
          }
        }
        else if (o.solver == 1)
        {
            for (int i = lane; i < n * n; i += 64) V[i] = H[i];
            __syncthreads();
            ldlt_solve(V, g, x, tmp, order, n, lane);
        }
        else
        {
            double *G = tmp + 2 * n; // third area, n x (n + 1) like V
            const int ld = n + 1;
            for (int i = lane; i < n * n; i += 64) G[(i / n) * ld + i % n] = H[i];
            __syncthreads();
            svd_solve(G, V, g, x, tmp, n, ld, lane);
        }
#if defined(MBAVO_EIG_STAMPS)
        ts3 = __builtin_amdgcn_s_memtime();
#endif
        for (int i = tid; i < n; i += T) x[i] = -x[i];
        __syncthreads();
        double gx = 0.0, xHx = 0.0; // every wave sums the whole vectors
        for (int r = lane; r < n; r += 64)
        {
            gx += g[r] * x[r];
            double a = 0.0;
            for (int c = 0; c < n; ++c) a += H[c * n + r] * x[c];
            xHx += x[r] * a;
        }
        gx = wsum(gx);
        xHx = wsum(xHx);
        s.model = -(gx + 0.5 * xHx);
        if (s.model < 0)
        { // handleInvalidStep
            lm_rejected(s);
            trace_push(s, tr, o.trace_cap, tid, s.level, 3, 0.0, s.model, 0.0);
            ++s.n_invalid;
            if (tid == 0) { active[e] = 0; states[b] = s; slot_publish(num_done, host_word, slot, B, false, pose_status); }
            return;
        }
        // computeCandidatePointAndEvaluateCost (:833-883): candidate = current (+) step, into the evaluated buffers
        double *Wt = const_cast<double *>(d.knots_t), *WR = const_cast<double *>(d.knots_R);
        // (a copy in LDS, V's place -- the solvers are done with it: the pose entries below read the candidate from there)
        double *Lt = V, *LR = V + 3 * N;
        for (int i = tid; i < 3 * N; i += T) { const double v = Ct[i] + x[i]; Wt[i] = v; Lt[i] = v; }
        for (int i = tid; i < N; i += T)
        {
            const Quat q = qmul(load_quat(CR + 4 * i), so3_exp(x + 3 * N + 3 * i)); // Spline.h:317-330, not re-normalised
            WR[4 * i] = q.x; WR[4 * i + 1] = q.y; WR[4 * i + 2] = q.z; WR[4 * i + 3] = q.w;
            LR[4 * i] = q.x; LR[4 * i + 1] = q.y; LR[4 * i + 2] = q.z; LR[4 * i + 3] = q.w;
        }
        if (tid == 0) { active[e] = 1; states[b] = s; slot_publish(num_done, host_word, slot, B, false, pose_status); }
        // The blur samples' pose entries of the candidate, WITH the knot Jacobians (round 4): the cost-only pass and -- if the
        // step is accepted -- the H/g pass of this slot evaluate at exactly these knots, so the entries are computed ONCE here,
        // by the workgroup that has the knots in its LDS, instead of by a pose launch / a pose prologue in each of the two passes
        // (Engine::set_external_poses; the arithmetic of k_pose_table: frame_pose_entries, one wave per knot).
        if constexpr (T >= 64 * KD)
        {
            if (pose_table != nullptr)
            {
                __syncthreads(); // the candidate is complete in LDS
                const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
                SplineSeg *segs = (SplineSeg *)(V + 8 * N); // (8-byte aligned; S x (KD - 1) segments: sized by the host)
                for (int f = 0; f < F; ++f)
                {
                    frame_pose_entries<KD, true>(d, Lt, LR, f, pose_table + d.pose_base + f * d.S, segs, wave, lane, pose_status, true);
                    __syncthreads(); // the next frame overwrites the segments
                }
            }
        }
#if defined(MBAVO_EIG_STAMPS)
        if (tid == 0 && b == 0)
            printf("k_lm_solve<%d,%d> block 0: merge %lld | damp + store %lld | solve %lld | model + candidate %lld cycles\n", KD, T, ts1 - ts0,
                   ts2 - ts1, ts3 - ts2, (long long)__builtin_amdgcn_s_memtime() - ts3);
#endif
    }

    // One wave per problem, after the cost-only pass on the candidates: step quality, accept / reject, outliers.
    template <int KD>
    __global__ __launch_bounds__(64) void k_lm_decide(const ProblemDesc *__restrict__ descs, LmState *__restrict__ states, LmOpts o,
                                                      FinSrc fs, const double *__restrict__ patch_cost,
                                                      double *__restrict__ inv,
                                                      double *__restrict__ cur_t, double *__restrict__ cur_R,
                                                      int *__restrict__ active, mbavo_trace_rec *__restrict__ trace,
                                                      int *__restrict__ num_done, unsigned long long *host_word2, int slot, int B)
    {
        constexpr int ND = 6 * KD + 1, E = ND * (ND + 1) / 2;
        const int b = blockIdx.x, lane = threadIdx.x;
        const int e = o.levels > 1 ? b * o.levels + states[b].level : b; // (the pair's entry, see k_lm_solve)
        const ProblemDesc &d = descs[e];
        int e_t0 = 0, e_t1 = 0;
        const bool early = fs.f1 && fs.deferred; // (see FinSrc::f1)
        if (early) { e_t0 = fs.tile_begin[e]; e_t1 = fs.tile_begin[e + 1]; }
        LmState s = states[b];
        if (s.done || active[e] != 1)
        { // finished, an invalid step, or a level switch (the new level's first H/g pass is next): no candidate was evaluated
            if (lane == 0) decide_publish(num_done, host_word2, slot, B, lm_will_finish(s, o));
            return;
        }
        mbavo_trace_rec *tr = trace ? trace + (size_t)b * o.trace_cap : nullptr;
        // the patch costs of frame 0 (up to kPre per lane) are fetched WITH the costs, before the accept test needs either: the
        // three statistics passes below then run from registers (same order of additions: bit-identical flags)
        constexpr int kPre = 8;
        const double *pc = patch_cost + d.patch_base;
        const bool pre = d.K <= 64 * kPre;
        double pcv[kPre];
#pragma unroll
        for (int q = 0; q < kPre; ++q) pcv[q] = (pre && lane + 64 * q < d.K) ? pc[lane + 64 * q] : 0.0;
        double cost = 0.0;
        if (early) cost = slot_sum_range(fs, e_t0, e_t1 - e_t0, E);
        else
            for (int f = 0; f < d.F; ++f) cost += slot_cost<E>(fs, d.bf_base + f);
        s.cand_cost = cost;
        s.abs_dec = s.eval_cost - s.cand_cost; // recorded before the accept test (:624)
        s.quality = tr_quality(s, s.cand_cost, s.model);
        if (s.quality > o.min_q && s.cand_cost < s.eval_cost)
        { // isStepSuccessful (:890-894) -> detectOutliersAndUploadToGpu (:639-699): patch costs of frame 0
            unsigned char *flags = const_cast<unsigned char *>(d.outlier);
            double sum = 0.0, cnt = 0.0, var = 0.0, nbad = 0.0;
            if (pre)
            {
#pragma unroll
                for (int q = 0; q < kPre; ++q)
                    if (lane + 64 * q < d.K && !(pcv[q] < 1e-8)) { sum += pcv[q]; cnt += 1.0; }
            }
            else
                for (int i = lane; i < d.K; i += 64)
                {
                    const double c = pc[i];
                    if (c < 1e-8) continue;
                    sum += c;
                    cnt += 1.0;
                }
            sum = wsum(sum);
            cnt = wsum(cnt);
            const double mu = sum / cnt;
            if (pre)
            {
#pragma unroll
                for (int q = 0; q < kPre; ++q)
                    if (lane + 64 * q < d.K && !(pcv[q] < 1e-8)) var += (pcv[q] - mu) * (pcv[q] - mu);
            }
            else
                for (int i = lane; i < d.K; i += 64)
                {
                    const double c = pc[i];
                    if (c < 1e-8) continue;
                    var += (c - mu) * (c - mu);
                }
            var = wsum(var) / cnt;
            const double bound = o.chi * (double)sqrtf((float)var);
            if (pre)
            {
#pragma unroll
                for (int q = 0; q < kPre; ++q)
                    if (lane + 64 * q < d.K && fabs(pcv[q] - mu) > bound) { flags[lane + 64 * q] = 1; nbad += 1.0; }
            }
            else
                for (int i = lane; i < d.K; i += 64)
                    if (fabs(pc[i] - mu) > bound) { flags[i] = 1; nbad += 1.0; }
            s.num_bad = (int)wsum(nbad);
            const long long num_residuals = (long long)(d.K - s.num_bad) * d.F * d.P;
            // accept: the candidate becomes the current point, the next pass re-evaluates H/g there
            double *Ct = cur_t + (size_t)b * 3 * o.max_N, *CR = cur_R + (size_t)b * 4 * o.max_N;
            for (int i = lane; i < 3 * d.N; i += 64) Ct[i] = d.knots_t[i];
            for (int i = lane; i < 4 * d.N; i += 64) CR[i] = d.knots_R[i];
            s.fresh = 1;
            s.pending_accept = 1;
            if (lane == 0)
            {
                inv[e] = num_residuals > 0 ? 1.0 / (double)num_residuals : 0.0;
                active[e] = 2;
                states[b] = s;
                decide_publish(num_done, host_word2, slot, B, lm_will_finish(s, o));
            }
            return;
        }
        lm_rejected(s); // handleUnsuccessfulStep
        trace_push(s, tr, o.trace_cap, lane, s.level, 2, s.cand_cost, s.model, s.quality);
        ++s.n_reject;
        if (lane == 0) { active[e] = 0; states[b] = s; decide_publish(num_done, host_word2, slot, B, lm_will_finish(s, o)); }
    }

    // ---- host driver.  lm_batch() = plan (everything decided from the arguments) -> arena (the layout) -> head upload, first
    // evaluation -> one of the two slot schedules -> collect; LmCallGuard restores the engine on every way out.
    // A failed runtime call: one line on stderr, the runtime's code returned (lm_batch maps it at its one exit).
    static int lm_hip(hipError_t e, const char *expr)
    {
        if (e != hipSuccess) fprintf(stderr, "mbavo lm_batch: %s failed: %s\n", expr, hipGetErrorString(e));
        return (int)e;
    }
#define LM_HIP(expr) do { if (const int e_ = lm_hip((expr), #expr)) return e_; } while (0)

    int lm_batch_check(int B, int L, const mbavo_problem *probs, const mbavo_lm_batch_opts &opt)
    {
        const int k = opt.spline_deg_k;
        if (B < 1 || L < 1 || L > 8 || !probs || (k != 2 && k != 4) || (opt.solver_type != 0 && opt.solver_type != 1) ||
            opt.max_num_iterations < 0)
            return MBAVO_E_ARG;
        for (int e = 0; e < B * L; ++e)
            if (probs[e].N < k || probs[e].N > 16 || !probs[e].h_start_idx || probs[e].F < 1) return MBAVO_E_ARG;
        // the levels of a pair are one spline seen at several resolutions: one knot buffer (updated in place, read by every level's
        // passes), one set of frames and times
        for (int b = 0; b < B; ++b)
            for (int l = 1; l < L; ++l)
            {
                const mbavo_problem &p = probs[(size_t)b * L + l], &q = probs[(size_t)b * L];
                if (p.F != q.F || p.N != q.N || p.t0 != q.t0 || p.dt != q.dt || p.huber_a != q.huber_a || p.d_cap_time != q.d_cap_time ||
                    p.d_exp_time != q.d_exp_time || p.d_knots_t != q.d_knots_t || p.d_knots_R != q.d_knots_R)
                    return MBAVO_E_ARG;
                for (int f = 0; f < p.F; ++f)
                    if (p.h_start_idx[f] != q.h_start_idx[f]) return MBAVO_E_ARG;
            }
        return 0;
    }

    // Everything a call decides before anything is allocated or launched; a function of its arguments only (no runtime call).
    struct LmCallPlan
    {
        LmOpts o;
        int B, L, k, E, NP, nbf = 0, max_S; // B pairs of L levels: the engine's list holds all NP = B L entries (pair-major), the LM kernels run one workgroup per pair
        long long total_K = 0, total_patches = 0;
        bool eig, ext_poses;  // the wide workgroup k_lm_solve<KD, kEigT>; ... which also leaves its candidates' pose entries in the engine's table
        size_t lds;           // of the solve kernel
        bool defer;           // defer_finalize = -1: the engine's finalize kernels write frame blocks and the LM kernels read those
        bool retile_allowed;  // as far as the arguments decide it: Passes::init has the engine's say
        int sync_every;       // <= 0: run_slots_pinned_words, > 0: run_slots_drained
        // a level of n iterations takes n + 1 solve launches (the last one ends it -- and, with levels, switches the pair to the next
        // level in the same slot); L (max_it + 2) slots bound every schedule
        int last_slot;
    };
    static int lm_plan(int B, int L, const mbavo_problem *probs, const mbavo_lm_batch_opts &opt, const EnvOverrides &env, const LmBatchShared *shared,
                       int trace_cap, LmCallPlan &p)
    {
        if (lm_batch_check(B, L, probs, opt) != 0) return MBAVO_E_ARG;
        const int k = opt.spline_deg_k;
        p.B = B; p.L = L; p.k = k; p.NP = B * L; p.E = (6 * k + 1) * (6 * k + 2) / 2;
        for (int b = 0; b < p.NP; ++b)
        {
            p.nbf += probs[b].F;
            p.total_K += probs[b].K > 0 ? probs[b].K : 1;
            p.total_patches += (long long)probs[b].F * probs[b].K;
        }
        LmBatchShared m = LmBatchShared::of(probs, p.NP);
        if (shared) m = {std::max(m.max_N, shared->max_N), std::max(m.max_S, shared->max_S)}; // (a group of a bigger batch: the batch's strides and kernel form)
        const int max_N = m.max_N, max_n = 6 * max_N;
        p.max_S = m.max_S;
        LmOpts &o = p.o;
        o.max_it = opt.max_num_iterations; o.max_nonmono = opt.max_consecutive_nonmonotonic_steps; o.solver = opt.solver_type;
        o.trace_cap = trace_cap; o.max_n = max_n; o.max_N = max_N;
        o.min_q = opt.min_step_quality; o.min_dec = opt.min_abs_cost_decrease; o.chi = opt.max_chi_square_error;
        o.levels = L;
        // the solver forms and the schedule of this call: mbavo_lm_batch_opts' tail under the environment's override layer (options.h)
        o.fast_ratio = opt_fast_ratio(opt.fast_solve_ratio, env.fast_solve);                 // default 1e8; 0: the Jacobi solvers / the pivoted LDL^T only
        o.refined_ratio = opt_refined_ratio(opt.refined_ratio, env.lm_refine, o.fast_ratio); // default 1e13; 0: the plain stand-in only
        // every system within the wide workgroup's reach (k_lm_solve<KD, kEigT>: solver 0 falls back to the workgroup-parallel
        // eigenvalue Jacobi there, solver 1 to the pivoted LDL^T on wave 0; both get their candidates' pose entries from it);
        // mbavo_lm_batch_opts.eig = -1 keeps the one-wave one-sided sweeps
        p.eig = max_n <= kEigMaxN && opt_flag(opt.eig, env.lm_eig, true);
        const size_t lds_solver = p.eig ? (eig_lds_doubles(max_n) + 3 * max_n + (size_t)max_n * max_n) * sizeof(double) + (size_t)(4 + 2 * max_n) * sizeof(int)
                                        : ((size_t)2 * max_n * (max_n + 1) + 6 * max_n) * sizeof(double) + (size_t)max_n * sizeof(int);
        // the solve kernel's pose entries (eigenvalue-Jacobi form only: it has the KD waves): candidate knots + the segments of
        // a frame's samples in the solvers' area
        p.ext_poses = p.eig && opt_flag(opt.pose_entries, env.lm_poses, true);
        const size_t lds_pose = p.ext_poses ? (size_t)8 * max_N * sizeof(double) + (size_t)(p.max_S < kPoseSPB ? p.max_S : kPoseSPB) * (k - 1) * sizeof(SplineSeg) : 0;
        p.lds = lds_solver > lds_pose ? lds_solver : lds_pose;
        if (p.lds > 160 * 1024) return MBAVO_E_ARG;
        p.defer = opt_flag(opt.defer_finalize, env.lm_defer, true);
        p.sync_every = opt.sync_every;
        p.last_slot = L * (o.max_it + 2) - 1;
        // retile = -1: one layout.  Levels (L > 1): one layout -- the fine tiling targets the whole list, not the active entries
        // of a set that mixes levels.
        p.retile_allowed = L == 1 && p.sync_every <= 0 && p.ext_poses && opt_flag(opt.retile, env.lm_retile, true);
        return 0;
    }

    // One arena for all LM state: the offsets, and typed pointers for a base -- the device arena, or the pinned copy of its head.
    struct LmArena
    {
        // head: what the host initialises, contiguous so that ONE copy from pinned memory uploads it (three pageable copies and
        // a fill of the whole arena cost ~35 us of a 64-pair call: four blit kernels with a ~6 us gap behind each); the initial
        // LM states ride in it: no init launch.  The rest is written before it is read: H, g by the first solve of a problem,
        // patch costs and frame blocks by the passes.
        size_t o_inv, o_act, o_done, o_start, o_flags, o_state, head_bytes, o_H, o_g, o_ct, o_cR, o_fb, o_pc, o_trace, bytes = 0;
        explicit LmArena(const LmCallPlan &p)
        {
            auto take = [&](size_t n) { const size_t at = bytes; bytes += (n + 255) & ~(size_t)255; return at; };
            const size_t B = p.B, max_n = p.o.max_n, max_N = p.o.max_N;
            o_inv = take(sizeof(double) * p.NP); o_act = take(sizeof(int) * p.NP); o_done = take(sizeof(int) * 16);
            o_start = take(sizeof(int) * p.nbf); o_flags = take((size_t)p.total_K); o_state = take(sizeof(LmState) * B);
            head_bytes = bytes;
            o_H = take(sizeof(double) * B * max_n * max_n); o_g = take(sizeof(double) * B * max_n);
            o_ct = take(sizeof(double) * B * 3 * max_N); o_cR = take(sizeof(double) * B * 4 * max_N);
            o_fb = take(sizeof(double) * (size_t)p.nbf * p.E); o_pc = take(sizeof(double) * (size_t)(p.total_patches + 1));
            o_trace = take(sizeof(mbavo_trace_rec) * B * p.o.trace_cap);
        }
        double *inv(char *b) const { return (double *)(b + o_inv); }          // [entry] 1 / num_residuals
        int *active(char *b) const { return (int *)(b + o_act); }             // [entry]
        int *num_done(char *b) const { return (int *)(b + o_done); }          // done counter, statistics, tickets
        int *start(char *b) const { return (int *)(b + o_start); }            // [slot] start indices
        unsigned char *flags(char *b) const { return (unsigned char *)(b + o_flags); }
        LmState *states(char *b) const { return (LmState *)(b + o_state); }   // [pair]
        double *H(char *b) const { return (double *)(b + o_H); }
        double *g(char *b) const { return (double *)(b + o_g); }
        double *cur_t(char *b) const { return (double *)(b + o_ct); }
        double *cur_R(char *b) const { return (double *)(b + o_cR); }
        double *frame_blocks(char *b) const { return (double *)(b + o_fb); }
        double *patch_costs(char *b) const { return (double *)(b + o_pc); }
        mbavo_trace_rec *trace(char *b) const { return (mbavo_trace_rec *)(b + o_trace); }
    };

    // The head in pinned memory, and in work[] every entry's outlier flags in the device arena at `dev`.
    static void fill_head(const LmCallPlan &p, const LmArena &a, std::vector<mbavo_problem> &work, char *dev, char *head)
    {
        memset(head, 0, a.head_bytes); // done counter, statistics, ticket and outlier flags start at zero
        size_t fo = 0;
        int bf = 0;
        for (int b = 0; b < p.NP; ++b)
        { // per-level reset of the outlier flags and count (:600-601): the engine owns them here (every entry has its own)
            work[b].d_outlier = a.flags(dev) + fo;
            work[b].num_bad = 0;
            fo += work[b].K > 0 ? work[b].K : 1;
            for (int f = 0; f < work[b].F; ++f) a.start(head)[bf++] = work[b].h_start_idx[f];
            // num_bad = 0 at the start of a level (:600); every problem takes part in the first H/g pass
            const long long num_residuals = (long long)work[b].K * work[b].F * work[b].P;
            a.inv(head)[b] = num_residuals > 0 ? 1.0 / (double)num_residuals : 0.0;
            a.active(head)[b] = b % p.L == p.L - 1 ? 2 : 0; // (levels: the pairs start at their coarsest entry)
        }
        for (int b = 0; b < p.B; ++b)
        {
            LmState &s0 = a.states(head)[b]; // (zero from the memset above)
            s0.radius = 1e4; s0.decrease_factor = 2.0; s0.abs_dec = 1e10; s0.fresh = 1; s0.level = p.L - 1;
        }
    }

    // MBAVO_LM_STAMPS=1: host-side phases of a call on stderr (development aid).  Unset: no clock is read inside the slot loop.
    struct LmStamps
    {
        using clock = std::chrono::steady_clock;
        const bool on = getenv("MBAVO_LM_STAMPS") && getenv("MBAVO_LM_STAMPS")[0] == '1';
        clock::time_point tp[6], sub[2];
        std::vector<double> slot_us; // per slot [solve launch | look-ahead wait | passes enqueued | solve word wait]
        void phase(int i) { if (on) tp[i] = clock::now(); }
        void first_eval(int i) { if (on) sub[i] = clock::now(); } // before / after the first Engine::evaluate
        double us() const { return on ? std::chrono::duration<double, std::micro>(clock::now() - tp[0]).count() : 0.0; }
        void slot(double t0, double t1, double t2, double t3) { if (on) slot_us.insert(slot_us.end(), {t1 - t0, t2 - t1, t3 - t2, us() - t3}); }
        void print(hipStream_t st, int B) const
        {
            if (!on) return;
            auto d = [](clock::time_point a, clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
            fprintf(stderr, "mbavo lm_batch:   first evaluation: %.1f us before the call (trace memset, words), %.1f us inside Engine::evaluate\n",
                    d(tp[2], sub[0]), d(sub[0], sub[1]));
            fprintf(stderr, "mbavo lm_batch: [stream %p, %d problems] host set-up %.1f us | head upload call %.1f | first evaluation enqueued %.1f | LM slots %.1f | results + drain %.1f\n",
                    (void *)st, B, d(tp[0], tp[1]), d(tp[1], tp[2]), d(tp[2], tp[3]), d(tp[3], tp[4]), d(tp[4], tp[5]));
            for (size_t i = 0; i + 3 < slot_us.size(); i += 4)
                fprintf(stderr, "mbavo lm_batch:   slot %zu: solve launch %.1f us | look-ahead wait %.1f | passes enqueued %.1f | solve word wait %.1f\n", i / 4,
                        slot_us[i], slot_us[i + 1], slot_us[i + 2], slot_us[i + 3]);
        }
    };

    // What the pieces of one call share.
    struct LmCall
    {
        const LmCallPlan &p;
        const LmArena &a;
        Engine &eng;
        std::vector<mbavo_problem> &work; // the list with the engine-owned outlier flags: the very list of every evaluate()
        char *dev, *pin;                  // the arena; pinned: [solve word, decide word, status at 32 (64 bytes) | head | final states]
        mbavo_trace_rec *trace;           // the caller's, may be null
        hipStream_t st;
        // the solve word (slot + 1, problems done) and the decide word (slot + 1, problems the next solve will end); pinned-word scheme
        volatile unsigned long long *h_word() const { return p.sync_every <= 0 ? (volatile unsigned long long *)pin : nullptr; }
        volatile unsigned long long *h_word2() const { return p.sync_every <= 0 ? (volatile unsigned long long *)pin + 1 : nullptr; }
        int *h_status() const { return (int *)(pin + 32); } // the engine's range-status counter lands here with the final states
        LmState *h_states() const { return (LmState *)(pin + 64 + a.head_bytes); } // (head_bytes is a multiple of 256)
        mbavo_trace_rec *d_trace() const { return trace ? a.trace(dev) : nullptr; }
    };

    // the solve kernel of a call, k_lm_solve<k, T>: T = kEigT threads (the eigenvalue-Jacobi form) or one wave
    template <class F>
    static decltype(auto) with_solve_kernel(const LmCallPlan &p, F f)
    {
        return dispatch<4, 2>(p.k, [&](auto KD) { return dispatch<true, false>(p.eig, [&](auto EIG) { return f(KD, std::integral_constant<int, EIG ? kEigT : 64>{}); }); });
    }
    static void launch_solve(const LmCall &c, const FinSrc &fs_hg, int slot)
    {
        const LmArena &a = c.a;
        // pinned host memory is device-visible at its own address
        unsigned long long *d_word = const_cast<unsigned long long *>(c.h_word());
        with_solve_kernel(c.p, [&](auto KD, auto T) {
            hipLaunchKernelGGL((k_lm_solve<KD, T>), dim3(c.p.B), dim3(T), c.p.lds, c.st, c.eng.device_descs(), a.states(c.dev), c.p.o, fs_hg, a.start(c.dev),
                               a.H(c.dev), a.g(c.dev), a.cur_t(c.dev), a.cur_R(c.dev), a.active(c.dev), c.d_trace(), a.num_done(c.dev), d_word, slot, c.p.B,
                               (PoseEntry<KD> *)(c.p.ext_poses ? c.eng.device_pose_table() : nullptr), c.eng.device_status(),
                               c.p.sync_every <= 0 && !c.trace ? c.h_states() : nullptr);
        });
    }
    static void launch_decide(const LmCall &c, const FinSrc &fs_cost, int slot)
    {
        const LmArena &a = c.a;
        // (the look-ahead word is only read for batches of up to 128 problems, see run_slots_pinned_words: bigger batches' decide
        // launches skip their B atomics on one address)
        unsigned long long *d_word2 = c.p.B <= 128 ? const_cast<unsigned long long *>(c.h_word2()) : nullptr;
        dispatch<4, 2>(c.p.k, [&](auto KD) {
            hipLaunchKernelGGL((k_lm_decide<KD>), dim3(c.p.B), dim3(64), 0, c.st, c.eng.device_descs(), a.states(c.dev), c.p.o, fs_cost, a.patch_costs(c.dev),
                               a.inv(c.dev), a.cur_t(c.dev), a.cur_R(c.dev), a.active(c.dev), c.d_trace(), a.num_done(c.dev), d_word2, slot, c.p.B);
        });
    }

    // The evaluation passes of a slot, the layout they go through and whose partials the LM kernels sum.
    // RE-TILING for the late slots of a big batch (round 4).  A batch of more pairs than CUs is tiled one tile per pair -- three
    // rounds of pixels per workgroup, the right grain while most pairs are active -- and a pass then lasts ~38 us as long as ONE
    // pair is active.  A second layout of the same list with four tiles per pair lives in the engine's companion (built while
    // the first evaluation runs); once few enough pairs are left that their fine tiles fit the CUs, both passes of a slot go
    // through it: one round per workgroup.  The LM kernels are told per launch whose partials to sum (FinSrc).
    struct Passes
    {
        const LmCall &c;
        Engine &eng;
        Engine *fine = nullptr;
        bool use_fine = false;            // the layout of the passes enqueued last
        FinSrc fs, fs_fine, fs_cost, fs_hg; // the two layouts'; whose partials the next decide / solve launch sums
        explicit Passes(const LmCall &call) : c(call), eng(call.eng) {}
        // after the first evaluation: it built the layout (device descriptors) the LM kernels read
        int init()
        {
            const LmCallPlan &p = c.p;
            fs.fb = c.a.frame_blocks(c.dev); fs.partials = eng.device_partials(); fs.tile_begin = eng.device_bf_tile_begin();
            fs.stride = p.E + 2; // engine.hip: Pack<k>::PSTRIDE
            fs.deferred = eng.finalize_deferred() ? 1 : 0;
            fs.f1 = p.nbf == p.NP ? 1 : 0; // (every F >= 1 was checked: nbf == NP means every F == 1)
            fs.inv = c.a.inv(c.dev);
            fs_fine = fs_hg = fs_cost = fs;
            if (!(p.retile_allowed && fs.deferred && eng.num_tiles() < 4 * p.nbf && eng.num_tiles() * 2 >= eng.num_cus())) return 0;
            fine = eng.companion();
            fine->set_tile_target(4ll * p.nbf);
            if (int r = fine->prepare(p.NP, c.work.data(), p.k, c.a.active(c.dev), c.a.inv(c.dev))) return r;
            if (fine->layout_flat() && fine->num_tiles() > eng.num_tiles())
            {
                fs_fine.partials = fine->device_partials();
                fs_fine.tile_begin = fine->device_bf_tile_begin();
                fs_fine.deferred = 1;
            }
            else
                fine = nullptr;
            return 0;
        }
        // cost-only pass on the candidates, decide, H/g pass on the accepted.  h_done: the count the previous slot's solve published
        int enqueue(int slot, int h_done)
        {
            const LmCallPlan &p = c.p;
            if (fine != nullptr && !use_fine && (long long)(p.B - h_done) * 4 <= eng.num_cus())
            {
                use_fine = true;
                fine->set_defer_finalize(true);
                fine->set_external_poses(true, eng.device_pose_table());
            }
            Engine &E = use_fine ? *fine : eng;
            fs_cost = use_fine ? fs_fine : fs;
            const bool same_list = p.sync_every <= 0; // (the drained scheme has the engine compare the list, as it always did)
            double *fb = c.a.frame_blocks(c.dev), *pc = c.a.patch_costs(c.dev), *inv = c.a.inv(c.dev);
            int *act = c.a.active(c.dev);
            if (int r = E.evaluate(p.NP, c.work.data(), p.k, false, fb, pc, nullptr, nullptr, act, inv, false, same_list)) return r;
            launch_decide(c, fs_cost, slot);
            const int r = E.evaluate(p.NP, c.work.data(), p.k, true, fb, pc, nullptr, nullptr, act, inv, false, same_list);
            fs_hg = fs_cost; // (the next solve launch sums this pass' partials)
            return r;
        }
    };

    // a pinned word did not arrive in 10 s: a launch failed or the device is wedged -- let the runtime say which
    static int lm_timed_out(hipStream_t st)
    {
        LM_HIP(hipStreamSynchronize(st));
        LM_HIP(hipGetLastError());
        return MBAVO_E_TIMEOUT; // (not MBAVO_E_RANGE: a wedged device is not an out-of-range capture time)
    }

    // sync_every <= 0 (default): the last workgroup of every solve launch stores (slot + 1, problems done) into a pinned host word
    // (slot_publish); the host enqueues slot i's solve AND its three passes, then spins on that word until solve i has been
    // published -- nothing but kernels is in the stream (the D2H copy + event of the previous scheme cost a 4.4 us blit kernel and
    // a 5.8 us gap behind it per slot: tools/lm_timeline.py).
    static int run_slots_pinned_words(const LmCall &c, Passes &ps, LmStamps &stamps, int &h_done)
    {
        volatile unsigned long long *h_word = c.h_word(), *h_word2 = c.h_word2();
        // the solve and decide words: slot number (high half) at least `slot`, waited for 10 s at the most
        auto wait_slot = [](volatile unsigned long long *word, int slot) {
            return wait_pinned_word(word, (unsigned long long)slot << 32, SpinBound{0, 10.0}, true);
        };
        const int B = c.p.B, last_slot = c.p.last_slot;
        for (int slot = 0;; ++slot)
        {
            const double ts0 = stamps.us();
            launch_solve(c, ps.fs_hg, slot);
            c.eng.set_external_poses(c.p.ext_poses); // from here on the passes read the entries the solve launches leave in the table
            // The three passes of this slot go in behind the solve BEFORE the host looks at the solve's word: the device has
            // ~45 us of work queued while the host waits.  Look-ahead: the PREVIOUS slot's decide launch has told how many
            // problems this solve will end (decide_publish; that launch retired at least a whole H/g pass ago by the time the
            // device gets here, so the wait below is for the host's own benefit, not the device's); if that is every one,
            // nothing is enqueued behind the solve.
            const bool last = slot == last_slot;
            bool ending = last;
            const double ts1 = stamps.us();
            // (batches of up to 128 problems only: a big batch's passes take the host 20-90 us to enqueue, which must overlap
            // the device's previous slot -- waiting for the decide word first cost the 512-pair call 54 us in bubbles for
            // 30 us of idle launches saved)
            if (!last && slot > 0 && B <= 128)
            {
                if (!wait_slot(h_word2, slot)) return lm_timed_out(c.st);
                ending = (int)(unsigned)(*h_word2 & 0xffffffffull) >= B;
            }
            const double ts2 = stamps.us();
            if (!ending)
                if (int r = ps.enqueue(slot, h_done)) return r;
            const double ts3 = stamps.us();
            const bool published = wait_slot(h_word, slot + 1);
            stamps.slot(ts0, ts1, ts2, ts3);
            if (!published) return lm_timed_out(c.st);
            h_done = (int)(unsigned)(*h_word & 0xffffffffull);
            if (h_done >= B || last) return 0;
            if (ending) // (the look-ahead over-counted: cannot happen, but never hang on it)
                if (int r = ps.enqueue(slot, h_done)) return r;
        }
    }

    // sync_every > 0: the host drains the stream and reads the done-counter every that many iterations (round 1's scheme: up to
    // sync_every - 1 iterations of idle launches after the last problem has finished, and a pipeline bubble at every read).
    static int run_slots_drained(const LmCall &c, Passes &ps, int &h_done)
    {
        const int n = c.p.sync_every, last_slot = c.p.last_slot;
        hipStream_t st = c.st;
        int *num_done = c.a.num_done(c.dev);
        for (int slot = 0; slot <= last_slot; ++slot)
        {
            launch_solve(c, ps.fs_hg, slot);
            c.eng.set_external_poses(c.p.ext_poses);
            if (slot % n == n - 1 || slot == last_slot)
            {
                LM_HIP(hipMemcpyAsync(&h_done, num_done, sizeof(int), hipMemcpyDeviceToHost, st));
                LM_HIP(hipStreamSynchronize(st));
                if (h_done >= c.p.B) break;
            }
            if (int r = ps.enqueue(slot, h_done)) return r; // (one layout here: the count is not looked at)
        }
        return 0;
    }

    // Final states, trace and range status to the host, then the call's results.
    static int collect(const LmCall &c, int h_done, LmStamps &stamps, mbavo_lm_batch_result *results)
    {
        const int B = c.p.B;
        hipStream_t st = c.st;
        int *h_status = c.h_status(), *num_done = c.a.num_done(c.dev);
        LM_HIP(hipGetLastError());
        if (c.p.sync_every <= 0 && !c.trace && h_done >= B)
        { // every problem's final state and the status counter are in pinned memory already (k_lm_solve, slot_publish); what is
          // still in flight is the tail of the last solve launch: poll the stream instead of a blocking wait (~20 us to wake up)
            const auto t_q = std::chrono::steady_clock::now();
            hipError_t q;
            while ((q = hipStreamQuery(st)) == hipErrorNotReady)
                if (std::chrono::steady_clock::now() - t_q > std::chrono::seconds(10)) break;
            if (q != hipSuccess) LM_HIP(hipStreamSynchronize(st));
            __atomic_thread_fence(__ATOMIC_ACQUIRE); // the device's release store of the word -> the final states and the status below
            *h_status = *reinterpret_cast<volatile int *>(c.h_word() + 4);
        }
        else
        {
            LM_HIP(hipMemcpyAsync(c.h_states(), c.a.states(c.dev), sizeof(LmState) * B, hipMemcpyDeviceToHost, st)); // pinned: no staging
            if (c.trace) LM_HIP(hipMemcpyAsync(c.trace, c.d_trace(), sizeof(mbavo_trace_rec) * (size_t)B * c.p.o.trace_cap, hipMemcpyDeviceToHost, st));
            if (int r = c.eng.fetch_status_enqueue(h_status)) return r; // (no blocking copy of its own after the drain: ~10 us)
            LM_HIP(hipStreamSynchronize(st));
        }
        stamps.phase(5);
        stamps.print(st, B);
        if (c.eng.fetch_status_take(h_status) != 0) return MBAVO_E_RANGE; // a capture time outside the spline somewhere in the call
        if (h_done < B)
        {
            LM_HIP(hipMemcpy(&h_done, num_done, sizeof(int), hipMemcpyDeviceToHost));
            if (h_done < B) return MBAVO_E_RANGE;
        }
        if (const char *e = getenv("MBAVO_LM_STATS"); e && e[0] == '1' && c.p.eig)
        {
            int st4[6] = {0, 0, 0, 0, 0, 0};
            LM_HIP(hipMemcpy(st4, num_done, sizeof(st4), hipMemcpyDeviceToHost));
            fprintf(stderr, "mbavo lm_batch: %d LDL^T stand-ins; %d eigenvalue-Jacobi solves, %.2f sweeps on average, %d at most, %d preconditioned (L^T L)\n",
                    st4[5], st4[1], st4[1] ? (double)st4[2] / st4[1] : 0.0, st4[3], st4[4]);
        }
        for (int b = 0; results && b < B; ++b)
        {
            const LmState &s = c.h_states()[b];
            mbavo_lm_batch_result &r = results[b];
            r.iterations = s.iter + s.iter_sum; r.accepted = s.n_accept; r.rejected = s.n_reject; r.invalid = s.n_invalid;
            r.num_outliers = s.num_bad; r.num_trace = s.ntrace;
            r.initial_cost = s.initial_cost; r.final_cost = s.eval_cost; r.radius = s.radius;
        }
        return 0;
    }

    // One call between the plan and the guard: arena, head upload, first evaluation, slots, results.  Returns 0, a negative
    // MBAVO_E_*, or a positive runtime error.
    static int lm_run(Engine &eng, const LmCallPlan &p, const mbavo_problem *probs, mbavo_lm_batch_result *results, mbavo_trace_rec *trace,
                      LmStamps &stamps)
    {
        hipStream_t st = eng.stream();
        const LmArena a(p);
        std::vector<mbavo_problem> work(probs, probs + p.NP);
        LM_HIP(hipSetDevice(eng.device()));
        // the engine's scratch slot 15, grown on demand and kept: no hipMalloc / hipFree per call (~90 us of a 64-pair call)
        char *dev = (char *)eng.named_scratch(kLmBatchSlot, a.bytes);
        char *pin = dev ? (char *)eng.pinned_scratch(kLmBatchPin, 64 + a.head_bytes + sizeof(LmState) * p.B) : nullptr;
        if (!pin) return (int)hipErrorOutOfMemory;
        const LmCall c{p, a, eng, work, dev, pin, trace, st};
        char *head = pin + 64;
        fill_head(p, a, work, dev, head);
        stamps.phase(1);
        LM_HIP(hipMemcpyAsync(dev, head, a.head_bytes, hipMemcpyHostToDevice, st));
        stamps.phase(2);
        if (trace) LM_HIP(hipMemsetAsync(c.d_trace(), 0, sizeof(mbavo_trace_rec) * (size_t)p.B * p.o.trace_cap, st));
        if (p.sync_every <= 0) { *c.h_word() = 0; *c.h_word2() = 0; } // (no kernel that writes them is in flight: every call ends with a stream synchronisation)
        eng.set_defer_finalize(p.defer);
        stamps.first_eval(0);
        // iteration 0 (:604): also builds the layout (device descriptors) the LM kernels read
        if (int r = eng.evaluate(p.NP, work.data(), p.k, true, a.frame_blocks(dev), a.patch_costs(dev), nullptr, nullptr, a.active(dev), a.inv(dev))) return r;
        stamps.first_eval(1);
        Passes ps(c);
        if (int r = ps.init()) return r;
        stamps.phase(3);
        if (p.lds > 48 * 1024) // more than 8 control knots: the three n x n areas need the large-LDS attribute
            LM_HIP(with_solve_kernel(p, [&](auto KD, auto T) { return hipFuncSetAttribute((const void *)k_lm_solve<KD, T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds); }));
        int h_done = 0;
        if (int r = p.sync_every <= 0 ? run_slots_pinned_words(c, ps, stamps, h_done) : run_slots_drained(c, ps, h_done)) return r;
        stamps.phase(4);
        return collect(c, h_done, stamps, results);
    }

    // On every way out of a call, what the next call and the engine's other users rely on.
    struct LmCallGuard
    {
        Engine &eng;
        const int &rc;
        ~LmCallGuard()
        {
            // an error exit may leave solve launches queued that still store into the pinned done word and the arena: drain them
            // before the next call re-arms the word or regrows either buffer
            if (rc != 0)
            {
                (void)hipStreamSynchronize(eng.stream());
                // range-status increments of the failed call must not be reported by the next, successful one: bring
                // the engine's `seen` count up to the device's counter
                (void)eng.fetch_status();
            }
            eng.set_external_poses(false);
            eng.set_defer_finalize(false);
            if (Engine *c = eng.companion_if_any()) { c->set_external_poses(false); c->set_defer_finalize(false); }
        }
    };

    int lm_batch(Engine &eng, int B, int L, const mbavo_problem *probs, const mbavo_lm_batch_opts &opt, mbavo_lm_batch_result *results,
                 mbavo_trace_rec *trace, int trace_cap, const LmBatchShared *shared)
    {
        LmStamps stamps;
        stamps.phase(0);
        LmCallPlan p;
        if (int r = lm_plan(B, L, probs, opt, read_env_overrides(), shared, trace ? trace_cap : 0, p)) return r;
        int rc = 0;
        const LmCallGuard guard{eng, rc};
        rc = lm_run(eng, p, probs, results, trace, stamps);
        return rc > 0 ? -1000 - rc : rc;
    }
} // namespace mbavo

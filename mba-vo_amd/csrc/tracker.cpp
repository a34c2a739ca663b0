// tracker.cpp -- coarse-to-fine Levenberg-Marquardt loop of the blur-aware tracker on the fused engine:
// BlurAwareDirectTracker::optimizeTrajectory / optimizePyramidLevel and the
// helpers they call (ba_tracker/blur_aware_direct_tracker.cpp:544-924).
//
// Control-flow details that decide how often the hot path runs and which step is taken
// are kept as in the reference: the damping H.diag += H.diag / radius is applied in
// place and therefore accumulates over rejected steps (:801-803); the model cost change
// uses the damped H (:821-823); abs_cost_decrease is recorded before the accept test, so
// any non-improving step ends the level (:624, :910-924); outlier statistics come from
// the patch costs of the candidate's cost-only pass, frame 0 only (:639-699); the LM
// radius and outlier flags are reset per level, the spline is warm-started (:590-606).
//
// optimize_trajectory() = plan (TrackPlan: everything decided from the arguments) -> buffers (TrackBuffers) -> the levels' problems
// -> one joint persistent kernel where the levels fit one -> run_level per level (LevelEval: one level's evaluations; RideAlong: the
// next level's first evaluation on the back of a candidate's command; PushLayout: the format of a slot's push block) -> knots
// back; TrackCallGuard ends every persistent kernel on every way out.
#include "tracker.h"
#include "host_math.h"
#include "se3_math.h"
#include "timing.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace mbavo
{
    // A failed runtime call: one line on stderr, the runtime's code returned (optimize_trajectory maps it at its one exit).
    static int trk_hip(hipError_t e, const char *what)
    {
        if (e != hipSuccess) fprintf(stderr, "mbavo tracker: %s failed: %s\n", what, hipGetErrorString(e));
        return (int)e;
    }

    // `shadow` (may be null): the flags in ordinary host memory (the persistent kernels' flag bytes live in write-combined device
    // memory, which the host cannot read back at speed); *newly = how many patches this call flagged for the first time
    static int detect_outliers(const double *patch_cost, int K, double chi, unsigned char *flags, unsigned char *shadow = nullptr,
                               int *newly = nullptr)
    { // :639-699
        double sum = 0.0;
        std::vector<double> kept;
        kept.reserve(K);
        for (int i = 0; i < K; ++i)
        {
            const double c = patch_cost[i];
            if (c < 1e-8) continue;
            kept.push_back(c);
            sum += c;
        }
        const double mu = sum / kept.size();
        double var = 0.0;
        for (double c : kept) var += (c - mu) * (c - mu);
        var = var / kept.size();
        const double bound = chi * (double)sqrtf((float)var);
        int n = 0, fresh = 0;
        for (int i = 0; i < K; ++i)
            if (std::fabs(patch_cost[i] - mu) > bound)
            {
                flags[i] = 1;
                ++n;
                if (shadow) { fresh += shadow[i] == 0; shadow[i] = 1; }
            }
        if (newly) *newly = shadow ? fresh : n;
        return n;
    }

    static size_t flag_room(const mbavo_level &L) { return (size_t)(L.K > 0 ? L.K : 1); } // a level's outlier flags, bytes

    // Everything a call decides once, from its arguments and the options alone: nothing here touches the device.
    struct TrackPlan
    {
        int k, F, N, n, E, num_levels;
        const mbavo_level *level[8]; // coarse to fine (:571-575): level[li] = levels[num_levels - li - 1]
        std::vector<int> start_idx;  // :549-560
        size_t maxK, sumK;           // flag_room: the largest level's, all levels'
        size_t pc_off[8];            // joint kernel: level li's first patch cost (the patches of the levels before it first)
        // mbavo_track_opts under the environment's override layer (options.h).  speculate: -1 on the persistent levels, 0 never, 1 on
        // every level; ride_waste (tests): every ride-along counts as taken at other knots -- the wasted path on every level
        int speculate;
        bool persist_levels, ride_along, ride_waste, resum;
        double fast_ratio; // once per call (mbavo_lm_batch does the same)
    };

    static int plan_call(const mbavo_track_opts &o, const mbavo_level *levels, int F, const double *h_cap, double t0, double dt, int N, TrackPlan &p)
    {
        const int k = o.spline_deg_k, ndim = 6 * k + 1;
        if ((k != 2 && k != 4) || F < 1 || N < k || o.num_levels < 1 || o.num_levels > 8) return MBAVO_E_ARG;
        p.k = k; p.F = F; p.N = N; p.n = 6 * N; p.E = ndim * (ndim + 1) / 2; p.num_levels = o.num_levels;
        p.start_idx.resize(F);
        for (int f = 0; f < F; ++f) p.start_idx[f] = spline_segment_index(h_cap[f], t0, dt); // :549-560
        p.maxK = 1; p.sumK = 0;
        size_t pc_off = 0;
        for (int li = 0; li < p.num_levels; ++li)
        {
            const mbavo_level &L = *(p.level[li] = &levels[p.num_levels - li - 1]);
            p.maxK = flag_room(L) > p.maxK ? flag_room(L) : p.maxK;
            p.sumK += flag_room(L);
            p.pc_off[li] = pc_off;
            pc_off += (size_t)F * L.K;
        }
        const EnvOverrides env = read_env_overrides(); // (options.h: the A/B tools' override layer over the options below)
        p.speculate = opt_tristate(o.speculate, env.speculate);
        p.persist_levels = opt_flag(o.persist_levels, env.persist_levels, true);
        p.ride_along = opt_flag(o.ride_along, env.ride_along, true);
        p.ride_waste = o.ride_along == 2;
        p.resum = opt_flag(o.resum, env.resum, true);
        p.fast_ratio = opt_fast_ratio(o.fast_solve_ratio, env.fast_solve);
        return 0;
    }

    // Engine-owned scratch, reused by every call (no hipMalloc / hipFree in the tracking loop).
    struct TrackBuffers
    {
        double *d_cap, *d_exp, *stage; // capture / exposure times on the device [cap F | exp F], and their pinned staging
        // the knots live in pinned, device-visible host memory [t (3N) | R (4N)]: the host writes them before an
        // evaluation and the kernels' pose prologue reads them over the bus -- no copy, no launch
        double *kt, *kR;
        // the per-patch costs land in pinned host memory (written by the fused kernel, read by detect_outliers after the
        // evaluation's synchronisation: no D2H copy); the flags are staged in pinned memory so that their upload is a
        // truly asynchronous copy
        // (sized for ALL levels side by side: one persistent kernel may serve every level of the call, see begin_joint)
        double *pc;
        unsigned char *flags, *d_flags;
        double *blocks, *inv; // pinned: frame blocks (zeroed); 1 / ((K - bad) F P), read by the kernels
    };

    static int take_buffers(Engine &eng, const TrackPlan &p, TrackBuffers &b)
    {
        const size_t n_blocks = (size_t)p.F * p.E * p.num_levels;
        b.d_cap = (double *)eng.named_scratch(kTimesSlot, sizeof(double) * 2 * p.F);
        b.kt = (double *)eng.pinned_scratch(kKnotsPin, sizeof(double) * 7 * p.N);
        b.pc = (double *)eng.pinned_scratch(kPatchCostPin, sizeof(double) * (size_t)p.F * p.sumK);
        b.flags = (unsigned char *)eng.pinned_scratch(kFlagsPin, p.maxK);
        b.d_flags = (unsigned char *)eng.named_scratch(kFlagsSlot, p.maxK);
        b.blocks = eng.host_frame_blocks(n_blocks); // device-visible pinned host memory
        b.inv = (double *)eng.pinned_scratch(kScalePin, sizeof(double));
        b.stage = (double *)eng.pinned_scratch(kTimesPin, sizeof(double) * 2 * p.F);
        if (!b.d_cap || !b.kt || !b.pc || !b.flags || !b.d_flags || !b.blocks || !b.inv || !b.stage) return (int)hipErrorOutOfMemory;
        b.d_exp = b.d_cap + p.F;
        b.kR = b.kt + 3 * p.N;
        memset(b.blocks, 0, sizeof(double) * n_blocks);
        return 0;
    }

    // A slot's push block behind Engine::kPushHeader -- fine-grained DEVICE memory the CPU writes through the PCIe BAR (write-only
    // for the host), where the per-evaluation inputs of a persistent kernel's workgroups live:
    //   [8 scale words | knots t (3N), R (4N) | joint form: the second knot area, the knots of a command's second problem | flags]
    // Per-level form (a kernel per level, in the level's slot): the scale in the first word, room for the largest level's flags.
    // Joint form (the levels are the problems of ONE kernel, slot 0): level li's scale in word li, its flags in 64-byte aligned
    // bytes of its own.  The one definition of the format: the host fills a block through it (LevelEval::take_block), the kernels
    // read it through the problems' pointers and the distance second_knot_area (engine.h).
    struct PushLayout
    {
        size_t scale[8], flags[8];   // level li's scale word (in doubles) and first flag byte (in bytes)
        size_t knots, knots2, bytes; // the knot areas (in doubles); the whole block, header included
        PushLayout(const TrackPlan &p, bool joint)
        {
            knots = 8;
            knots2 = knots + second_knot_area(p.N);
            size_t end = sizeof(double) * ((joint ? knots2 : knots) + 3 * (size_t)p.N + 4 * (size_t)p.N);
            for (int li = 0; li < p.num_levels; ++li)
            {
                scale[li] = joint ? li : 0;
                flags[li] = end;
                if (joint) end += (flag_room(*p.level[li]) + 63) & ~(size_t)63;
            }
            bytes = Engine::kPushHeader + end + (joint ? 0 : p.maxK) + 64;
        }
    };

    // THE NEXT LEVEL'S FIRST EVALUATION RIDES ALONG (round 5; mbavo_track_opts.ride_along, default on, joint persistent kernel
    // only).  A level almost always ends with a rejected candidate (A16: abs_dec goes negative), i.e. at the knots it had BEFORE
    // that candidate -- which are known when the candidate is posted.  So every candidate's command also names the next finer
    // level as its second problem, evaluated with H / g at the CURRENT knots by that level's own, otherwise idle, workgroups.  If
    // the level then ends at those very knots (compared bit for bit), the next level's iteration 0 is already there: one
    // dependent evaluation (~13.5 us) less per pyramid level.  A wasted ride-along costs idle GPU time, never a result.
    struct RideAlong
    {
        Engine &eng;
        const TrackPlan &plan;
        const SLAM::Core::SplineSE3 &cur; // the loop's current point
        std::vector<double> kt, kR;       // the knots the last ride-along was taken at
        int level = -1;                   // the level (li) the last ride-along evaluated, or -1
        unsigned long long seq = 0;       // ... and the sequence number of its command
        RideAlongStats &stats = RideAlongStats::get();

        // Level li's command about to be posted takes level li + 1 along as its second problem, at the CURRENT point, written to the
        // second knot area `area2` (null: not on the joint kernel).  Returns that problem, or -1: none goes along.
        int attach(int li, double *area2)
        {
            if (!area2 || !plan.ride_along || li + 1 >= plan.num_levels || plan.level[li + 1]->K <= 0) return -1;
            // (a new ride-along only behind a finished one: its workgroups must not miss a command that concerns them)
            if (level >= 0 && !eng.persistent_second_done(seq)) return -1;
            memcpy(area2, cur.get_knot_data_t(), sizeof(double) * 3 * plan.N);
            memcpy(area2 + 3 * plan.N, cur.get_knot_data_R(), sizeof(double) * 4 * plan.N);
            memcpy(kt.data(), cur.get_knot_data_t(), sizeof(double) * 3 * plan.N);
            memcpy(kR.data(), cur.get_knot_data_R(), sizeof(double) * 4 * plan.N);
            return li + 1;
        }
        void posted(int second) { level = second; seq = eng.posted_seq(); stats.posts.fetch_add(1, std::memory_order_relaxed); }
        // level li starts: its iteration 0 was evaluated by the last ride-along, at these very knots
        bool claim(int li) const
        {
            return level == li && !plan.ride_waste && memcmp(kt.data(), cur.get_knot_data_t(), sizeof(double) * 3 * plan.N) == 0 &&
                   memcmp(kR.data(), cur.get_knot_data_R(), sizeof(double) * 4 * plan.N) == 0;
        }
        // A ride-along taken at other knots may still be running on level li's workgroups.  Its tiles share the level's
        // ticket counters, tile partials and frame blocks with the command posted next, and the workgroups take commands
        // independently -- one could finish its wasted tile and bump the ticket for the NEW command while a sibling is still
        // on the old one (with two tiles: the first workgroup would count 0->1, 1->2 and sum its new partial with the
        // sibling's stale one).  So the wasted ride-along is waited out (<= one evaluation, ~10 us, on levels that end on an
        // accepted candidate only) before this level's first command goes out.
        int wait_out(int li)
        {
            if (level != li) return 0;
            PhaseScope ps(PhaseTimers::kWait);
            if (const int r = eng.persistent_wait_second(seq)) return r;
            stats.waits.fetch_add(1, std::memory_order_relaxed);
            return 0;
        }
    };

    // What is fixed for one level's evaluations: its problem, where the inputs of an evaluation go (its slot's push block on a
    // persistent kernel; pinned host memory / device copies where every evaluation is its own launch), where its frame blocks and
    // patch costs land, and the engine's (slot, problem) pair -- (0, li) on the joint kernel, (li, 0) on a kernel of its own.
    struct LevelEval
    {
        Engine *eng;
        const TrackPlan *plan;
        const mbavo_level *L;
        int li, slot, prob;
        mbavo_problem p; // (its knots and flags: where the level's inputs are at the time)
        double *w_inv, *w_kt, *w_kR, *w_kt2; // scale word, knots, second knot area (joint kernel only)
        unsigned char *w_flags;
        double *blocks, *pc;
        bool pushed, launched, persistent;

        // The outlier count changes with every accepted step; it reaches the kernels through a word (inv_ptr) instead of the
        // problem descriptor, so the engine's cached layout stays valid for the whole level
        void set_scale(int num_bad)
        {
            const long long nres = (long long)(L->K - num_bad) * plan->F * L->P; // spline_update_step.cpp:116-117
            *w_inv = nres > 0 ? 1.0 / (double)nres : 0.0;
        }
        // the level's inputs move into a push block of layout `lay`: no outliers (:601), the scale that goes with that
        void take_block(char *push, const PushLayout &lay, bool joint)
        {
            double *b = (double *)(push + Engine::kPushHeader);
            w_inv = b + lay.scale[li]; w_kt = b + lay.knots; w_kR = w_kt + 3 * plan->N; w_kt2 = joint ? b + lay.knots2 : nullptr;
            w_flags = (unsigned char *)b + lay.flags[li];
            p.d_knots_t = w_kt; p.d_knots_R = w_kR; p.d_outlier = w_flags;
            memset(w_flags, 0, flag_room(*L));
            set_scale(0);
        }
        // One evaluation at the given knots = post + finish: knots into the level's input buffer, ONE launch for these problem sizes
        // (pose prologue + fused + last-workgroup finalize; a command where the kernel is resident) whose frame blocks land in
        // pinned host memory, then a spin on the kernel's completion word: no copies, no stream synchronisation.  With `ride`
        // the command may take the next level along.  Nothing else is written to the slot's block until finish() returns.
        int post(const double *kt, const double *kR, bool with_h, RideAlong *ride = nullptr)
        {
            PhaseScope ps(PhaseTimers::kEnqueue);
            memcpy(w_kt, kt, sizeof(double) * 3 * plan->N);
            memcpy(w_kR, kR, sizeof(double) * 4 * plan->N);
            if (!persistent) return eng->evaluate(1, &p, plan->k, with_h, blocks, pc, nullptr, nullptr, nullptr, w_inv, true);
            const int second = ride ? ride->attach(li, w_kt2) : -1;
            const int r = eng->persistent_post(slot, with_h, prob, second);
            if (second >= 0) ride->posted(second);
            return r;
        }
        // wait (`wait`: the engine's call for what was posted), then the level's frame blocks merged into cost, H and g (null: cost only)
        template <class Wait> int wait_merge(Wait wait, double *cost, double *H, double *g) const
        {
            int r;
            {
                PhaseScope ps(PhaseTimers::kWait);
                r = wait();
            }
            if (r) return r;
            PhaseScope ps(PhaseTimers::kMerge);
            merge_blocks_host(plan->F, plan->k, blocks, plan->start_idx.data(), plan->N, cost, H, g);
            return 0;
        }
        int finish(bool with_h, double *cost, double *H, double *g) const
        {
            return wait_merge([this] { return persistent ? eng->persistent_wait() : eng->wait_evaluation(); }, cost, with_h ? H : nullptr, with_h ? g : nullptr);
        }
        int evaluate(const double *kt, const double *kR, bool with_h, double *cost, double *H, double *g, RideAlong *ride = nullptr)
        {
            if (const int r = post(kt, kR, with_h, ride)) return r;
            return finish(with_h, cost, H, g);
        }
        // the candidate's evaluation (this level's last command, with H / g) summed again under the flags and the scale as they are now
        bool resum_ok() const { return persistent && eng->persistent_resum_ok(slot, prob); }
        int evaluate_again(double *cost, double *H, double *g) const
        {
            const int r = eng->persistent_post_resum(slot, prob);
            return r ? r : wait_merge([this] { return eng->persistent_wait(); }, cost, H, g);
        }
    };

    struct TraceLog
    { // counts every record, keeps those that fit
        mbavo_trace_rec *recs;
        int cap, n;
        void add(int level, int iter, int kind, int num_bad, double radius, double eval_cost, double cc, double model, double q)
        {
            if (recs && n < cap) recs[n] = mbavo_trace_rec{level, iter, kind, num_bad, radius, eval_cost, cc, model, q};
            ++n;
        }
    };

    // computeTrustRegionStep (:799-831): damps H IN PLACE, solves for the step, returns the model cost change through `model`
    // (from the damped H, :821-823); < 0: the solver refused the system
    static int trust_region_step(std::vector<double> &H, const std::vector<double> &g, int n, double radius, int solver_type, double fast_ratio,
                                 std::vector<double> &step, double &model)
    {
        PhaseScope ps_solve(PhaseTimers::kSolve);
        const double iradius = 1. / radius;
        for (int i = 0; i < n; ++i) H[(size_t)i * n + i] += H[(size_t)i * n + i] * iradius;
        if (solve_normal_equation_host(H.data(), g.data(), n, solver_type, step.data(), fast_ratio) < 0) return MBAVO_E_ARG;
        double gx = 0.0, xHx = 0.0;
        for (int i = 0; i < n; ++i) gx += g[i] * step[i];
        for (int r = 0; r < n; ++r)
        {
            double a = 0.0;
            for (int c = 0; c < n; ++c) a += H[(size_t)c * n + r] * step[c];
            xHx += step[r] * a;
        }
        model = -(gx + 0.5 * xHx);
        return 0;
    }

    // One call's state: what the levels share.
    struct TrackCall
    {
        Engine &eng;
        const mbavo_track_opts &o;
        const TrackPlan &plan;
        TrackBuffers buf;
        LevelEval runs[8];
        bool joint;
        SLAM::Core::SplineSE3 spline;
        std::vector<double> H, g, step, cand_t, cand_R, Hs, gs; // Hs, gs: the candidate's H / g under speculation (run_level)
        std::vector<unsigned char> shadow;
        SLAM::VO::LevenbergMarquardtStrategy lm;
        SLAM::VO::TrustRegionStepEvaluator evaluator;
        double eval_cost;
        RideAlong ride;
        TraceLog trace;

        // (the vectors are sized here, once per call; Hs / gs only where some level may speculate)
        TrackCall(Engine &e, const mbavo_track_opts &opts, const TrackPlan &p, double t0, double dt, mbavo_trace_rec *recs, int cap)
            : eng(e), o(opts), plan(p), buf{}, joint(false), spline(t0, dt), H((size_t)p.n * p.n), g(p.n), step(p.n), cand_t(3 * (size_t)p.N),
              cand_R(4 * (size_t)p.N), Hs(p.speculate != 0 ? H.size() : 0), gs(p.speculate != 0 ? p.n : 0),
              evaluator(opts.max_consecutive_nonmonotonic_steps), eval_cost(0.0),
              ride{e, p, spline, std::vector<double>(3 * (size_t)p.N), std::vector<double>(4 * (size_t)p.N)}, trace{recs, cap, 0}
        {
        }
        int describe_levels(const double *h_cap, const double *h_exp, double t0, double dt);
        void push_level(int li);
        int launch(int li, bool cached_only);
        int begin_joint();
        int run_level(int li);
    };

    // The problem descriptor of every level, its inputs in the per-evaluation buffers; MBAVO_E_RANGE before anything is enqueued.
    int TrackCall::describe_levels(const double *h_cap, const double *h_exp, double t0, double dt)
    {
        memset(runs, 0, sizeof(runs));
        for (int li = 0; li < plan.num_levels; ++li)
        {
            const mbavo_level &L = *plan.level[li];
            const int scale = 1 << (plan.num_levels - li - 1);
            LevelEval &R = runs[li];
            R.eng = &eng; R.plan = &plan; R.L = &L; R.li = li; R.slot = li; R.prob = 0; R.blocks = buf.blocks; R.pc = buf.pc;
            mbavo_problem &p = R.p;
            p.S = L.S; p.F = plan.F; p.K = L.K; p.P = L.P; p.N = plan.N; p.H = L.H; p.W = L.W;
            p.d_ref_img = L.d_ref_img; p.d_ref_dIxy = L.d_ref_dIxy; p.d_cur_imgs = L.d_cur_imgs;
            p.d_kp_xy = L.d_kp_xy; p.kp_stride = 2; p.d_kp_z = L.d_kp_z; p.d_pattern = L.d_pattern;
            p.d_outlier = buf.d_flags; p.num_bad = 0;
            for (int a = 0; a < 4; ++a) p.intrinsics[a] = o.intrinsics[a] / scale; // :766-770
            p.d_cap_time = buf.d_cap; p.d_exp_time = buf.d_exp; p.t0 = t0; p.dt = dt;
            p.d_knots_t = buf.kt; p.d_knots_R = buf.kR; p.h_start_idx = plan.start_idx.data(); p.huber_a = o.huber_k;
            // every blur sample must fall on knots that exist (the reference reads past its arrays otherwise,
            // SplineFunctor.h:13-19).  The sample times depend on (cap, exp, S) only: checked here on the host with the
            // kernels' own formula instead of reading the device's status counter back (a synchronous copy per level:
            // 30 us, 12 % of a tracked frame)
            for (int f = 0; f < plan.F; ++f)
                for (int smp = 0; smp < L.S; ++smp)
                {
                    const double ts = h_cap[f] - h_exp[f] * 0.5 + smp * h_exp[f] / (L.S - 1 + 1e-8); // compute_virtual_camera_poses.cu:33
                    int idx;
                    double u;
                    if (!spline_segment_checked(ts, t0, dt, plan.N, plan.k, idx, u)) return MBAVO_E_RANGE;
                }
        }
        return 0;
    }

    // level li's inputs into its own slot's block, where the platform has one (once; a level without one evaluates by launches)
    void TrackCall::push_level(int li)
    {
        if (runs[li].pushed) return;
        const PushLayout lay(plan, false);
        if (char *push = (char *)eng.push_block(li, lay.bytes)) runs[li].take_block(push, lay, false);
        runs[li].pushed = true;
    }
    // enqueue level li's persistent kernel: 0 = enqueued, 1 = not applicable (now), otherwise an error
    int TrackCall::launch(int li, bool cached_only)
    {
        LevelEval &R = runs[li];
        if (R.launched) return 0;
        if (!R.w_inv) return 1;
        PhaseScope ps_level(PhaseTimers::kLevel);
        const int pr = eng.persistent_begin(li, R.p, plan.k, buf.blocks, buf.pc, R.w_inv, cached_only);
        if (pr == 0) R.launched = true;
        return pr;
    }

    // ONE persistent kernel for ALL levels of the call where they fit one list (round 3: a launch and a level set-up cost the
    // host ~14 us each, only partly hidden behind evaluations; trackFrame 0.366 -> see profiles/r03_kfused_experiments.txt 7.):
    // the levels are the problems of one layout, they share the knot buffer of slot 0's push block, every level has its own
    // scale word and flag bytes there, and a command names its level.  mbavo_track_opts.persist_levels = -1 keeps one kernel per level.
    int TrackCall::begin_joint()
    {
        joint = false;
        if (plan.num_levels <= 1 || !plan.persist_levels) return 0;
        const PushLayout lay(plan, true);
        char *push = (char *)eng.push_block(0, lay.bytes);
        if (!push) return 0;
        mbavo_problem lp[8];
        for (int li = 0; li < plan.num_levels; ++li)
        {
            runs[li].take_block(push, lay, true);
            lp[li] = runs[li].p;
        }
        PhaseScope ps_level(PhaseTimers::kLevel);
        const int pr = eng.persistent_begin(0, plan.num_levels, lp, plan.k, buf.blocks, buf.pc, runs[0].w_inv, false);
        if (pr < 0 || pr > 1) return pr;
        joint = pr == 0;
        for (int li = 0; li < plan.num_levels; ++li)
        {
            LevelEval &R = runs[li];
            if (!joint) { R.w_inv = R.w_kt2 = nullptr; continue; } // per-level kernels: their own slots (push_level)
            R.slot = 0; R.prob = li; R.persistent = true;
            R.blocks = buf.blocks + (size_t)li * plan.F * plan.E; // this level's frame blocks / patch costs
            R.pc = buf.pc + plan.pc_off[li];
        }
        return 0;
    }

    // One run of a pyramid level (optimizePyramidLevel, :590-637).  Small levels (everything the reference's semi-dense detector
    // produces) are ONE persistent launch each -- the evaluations are commands to its resident workgroups
    // (Engine::persistent_*) whose inputs live in the level's push block (PushLayout).  The kernel of level li + 1 is enqueued
    // while the first evaluation of level li is in flight (its launch cost hides behind that evaluation, and it starts the
    // moment level li's kernel exits).  Without a push block (or for levels too large for the sample-parallel kernel) the
    // inputs stay in pinned host memory / device copies and every evaluation is its own launch.
    int TrackCall::run_level(int li)
    {
        LevelEval &R = runs[li];
        const mbavo_level &L = *R.L;
        const int lv = plan.num_levels - li - 1, N = plan.N;
        memset(buf.flags, 0, flag_room(L)); // :601 (the device copy below, where it is used)
        shadow.assign(flag_room(L), 0);
        if (!joint)
        {
            push_level(li);
            const int pr = launch(li, false);
            if (pr < 0 || pr > 1) return pr;
            R.persistent = R.launched;
        }
        int num_bad = 0;
        if (!R.persistent)
        { // per-evaluation launches read the pinned knots and the device copy of the flags
            R.w_inv = buf.inv; R.w_kt = buf.kt; R.w_kR = buf.kR; R.w_flags = buf.flags;
            R.p.d_knots_t = buf.kt; R.p.d_knots_R = buf.kR; R.p.d_outlier = buf.d_flags;
        }
        R.set_scale(num_bad);
        if (!R.persistent)
            if (const int e = trk_hip(hipMemsetAsync(buf.d_flags, 0, flag_room(L), eng.stream()), "hipMemsetAsync(flags)")) return e;
        // Speculation (mbavo_track_opts.speculate): the candidate is evaluated WITH H / g.  An accepted step is followed by an H / g evaluation
        // at the very same knots (:896-903); it differs from the candidate's only through the outlier flags and the residual scale
        // detectOutliers may have changed in between (:639-699) -- where it changed neither, the candidate's H, g and cost ARE that
        // evaluation's, bit for bit, and it is skipped.
        // Worth it where an evaluation is latency-bound and H / g cost little more than the cost alone: the levels that run on
        // persistent kernels (trackFrame 0.330 -> 0.322 ms per frame, 172 -> 154 evaluations of 12.8 / 14.2 us over 8 tracked
        // frames, identical records and poses); dense levels pay twice the cost-only pass for a one-in-three hit.
        // mbavo_track_opts.speculate = -1 / 1: never / on every level.
        const bool speculate = plan.speculate == 1 || (plan.speculate < 0 && R.persistent);
        int r;

        // iteration 0 -- already evaluated by the previous level's last ride-along if that was taken at these very knots
        if (ride.claim(li))
        {
            if ((r = R.wait_merge([this] { return eng.persistent_wait_second(ride.seq); }, &eval_cost, H.data(), g.data()))) return r;
            ride.stats.hits.fetch_add(1, std::memory_order_relaxed);
        }
        else
        {
            if ((r = ride.wait_out(li))) return r;
            if ((r = R.post(spline.get_knot_data_t(), spline.get_knot_data_R(), true))) return r;
            if (R.persistent && !joint && li + 1 < plan.num_levels)
            { // with this level's first evaluation in flight: the next level's kernel goes into the queue (only if its layout
              // is one of the engine's parked ones -- nothing may be built or uploaded behind a running persistent kernel;
              // otherwise it is launched when its turn comes)
                push_level(li + 1);
                const int pr = launch(li + 1, true);
                if (pr < 0 || pr > 1) return pr;
            }
            if ((r = R.finish(true, &eval_cost, H.data(), g.data()))) return r;
        }
        if (ride.level == li) ride.level = -1;
        lm.reset();
        evaluator.reset(eval_cost);
        trace.add(lv, 0, 0, num_bad, lm.get_radius(), eval_cost, 0.0, 0.0, 0.0);

        int iter = 0;
        double abs_dec = 1e10;
        for (;;)
        {
            ++iter; // finalizeIterationAndCheckIfMinimizerCanContinue (:910-924)
            if (iter > o.max_num_iterations) break;
            if (abs_dec < o.min_abs_cost_decrease) break;

            // computeTrustRegionStep (:799-831)
            double model = 0.0;
            if ((r = trust_region_step(H, g, plan.n, lm.get_radius(), o.solver_type, plan.fast_ratio, step, model))) return r;
            if (model < 0) { lm.step_rejected(); trace.add(lv, iter, 3, num_bad, lm.get_radius(), eval_cost, 0.0, model, 0.0); continue; } // handleInvalidStep

            // computeCandidatePointAndEvaluateCost (:833-883)
            spline.Plus_t(step.data(), cand_t.data());
            spline.Plus_R(step.data() + 3 * N, cand_R.data());
            double cand_cost = 0.0;
            if ((r = R.evaluate(cand_t.data(), cand_R.data(), speculate, &cand_cost, Hs.data(), gs.data(), &ride))) return r;

            abs_dec = eval_cost - cand_cost;
            const double quality = evaluator.StepQuality(cand_cost, model);
            if (quality > o.min_step_quality && cand_cost < eval_cost)
            { // isStepSuccessful (:890-894) -> detectOutliers + handleSuccessfulStep (:896-903)
                bool same_inputs = false;
                {
                    PhaseScope ps(PhaseTimers::kOutliers);
                    const int bad_before = num_bad;
                    int newly = 0;
                    num_bad = detect_outliers(R.pc, L.K, o.max_chi_square_error, R.w_flags, shadow.data(), &newly); // frame 0's costs, just written
                    same_inputs = newly == 0 && num_bad == bad_before; // flags and residual scale as the candidate's evaluation saw them
                    if (PhaseTimers::get().on) ++PhaseTimers::get().calls[!same_inputs ? PhaseTimers::kFlagsChanged : PhaseTimers::kFlagsSame];
                    R.set_scale(num_bad);
                    if (!R.persistent)
                        if (const int e = trk_hip(hipMemcpyAsync(buf.d_flags, R.w_flags, L.K, hipMemcpyHostToDevice, eng.stream()), "hipMemcpyAsync(flags)")) return e;
                }
                spline.InvalidParameter(cand_t.data(), cand_R.data());
                // THE ACCEPTED STEP'S EVALUATION AS A RE-SUMMATION (round 5; mbavo_track_opts.resum, default on, persistent kernels).  Two of
                // three accepted steps flag new outliers, so the candidate's H / g (speculation above) are not the accepted point's -- but
                // they differ from it only in which patches' rows count and in the residual scale: the kernel's workgroups still hold the
                // candidate's per-patch sums and add them up again under the new flags (Engine::persistent_post_resum) -- the evaluation's
                // result bit for bit, without pose entries, taps and Jacobians.
                if (speculate && same_inputs)
                { // the candidate's evaluation IS the accepted point's
                    H.swap(Hs);
                    g.swap(gs);
                    eval_cost = cand_cost;
                }
                else if (speculate && plan.resum && R.resum_ok()) r = R.evaluate_again(&eval_cost, H.data(), g.data());
                else r = R.evaluate(spline.get_knot_data_t(), spline.get_knot_data_R(), true, &eval_cost, H.data(), g.data());
                if (r) return r;
                lm.step_accepted(quality);
                evaluator.StepAccepted(eval_cost, model);
                trace.add(lv, iter, 1, num_bad, lm.get_radius(), eval_cost, cand_cost, model, quality);
                continue;
            }
            lm.step_rejected(); // handleUnsuccessfulStep
            trace.add(lv, iter, 2, num_bad, lm.get_radius(), eval_cost, cand_cost, model, quality);
        }
        if (!joint) (void)eng.persistent_end(li); // the level's resident workgroups exit; the next level's kernel is already queued behind them
        return 0;
    }

    // On every way out of a call: no persistent kernel of it stays resident (per-level kernels end with their level, the joint one
    // with the call, on an error whatever is there).
    struct TrackCallGuard
    {
        Engine &eng;
        ~TrackCallGuard() { (void)eng.persistent_end_all(); }
    };

    // buffers -> the levels' problems -> times -> joint kernel -> the levels, coarse to fine (:571-575) -> knots back; 0 or the first error
    static int run_call(TrackCall &c, const double *h_cap, const double *h_exp, double t0, double dt, double *knots_t, double *knots_R, double *final_cost)
    {
        const TrackPlan &p = c.plan;
        if (int r = trk_hip(hipSetDevice(c.eng.device()), "hipSetDevice")) return r;
        if (int r = take_buffers(c.eng, p, c.buf)) return r;
        if (int r = c.describe_levels(h_cap, h_exp, t0, dt)) return r;
        // capture / exposure times: one asynchronous copy from pinned staging [cap F | exp F] (:701-719)
        memcpy(c.buf.stage, h_cap, sizeof(double) * p.F);
        memcpy(c.buf.stage + p.F, h_exp, sizeof(double) * p.F);
        if (int r = trk_hip(hipMemcpyAsync(c.buf.d_cap, c.buf.stage, sizeof(double) * 2 * p.F, hipMemcpyHostToDevice, c.eng.stream()), "hipMemcpyAsync(times)")) return r;
        if (int r = c.begin_joint()) return r;
        for (int li = 0; li < p.num_levels; ++li)
            if (int r = c.run_level(li)) return r;
        memcpy(knots_t, c.spline.get_knot_data_t(), sizeof(double) * 3 * p.N);
        memcpy(knots_R, c.spline.get_knot_data_R(), sizeof(double) * 4 * p.N);
        if (final_cost) *final_cost = c.eval_cost;
        return 0;
    }

    int optimize_trajectory(Engine &eng, const mbavo_track_opts &o, const mbavo_level *levels, int F,
                            const double *h_cap, const double *h_exp, double t0, double dt, double *knots_t,
                            double *knots_R, int N, int *start_idx_out, double *final_cost, mbavo_trace_rec *trace,
                            int trace_cap)
    {
        TrackPlan plan;
        if (int r = plan_call(o, levels, F, h_cap, t0, dt, N, plan)) return r;
        if (start_idx_out) memcpy(start_idx_out, plan.start_idx.data(), sizeof(int) * F);
        TrackCall c(eng, o, plan, t0, dt, trace, trace_cap);
        c.spline.setSplineDegK(plan.k);
        for (int i = 0; i < N; ++i) c.spline.InsertControlKnot(knots_R + 4 * i, knots_t + 3 * i);
        const TrackCallGuard guard{eng};
        const int rc = run_call(c, h_cap, h_exp, t0, dt, knots_t, knots_R, final_cost);
        return rc ? (rc > 0 ? -1000 - rc : rc) : c.trace.n; // a runtime error code (> 0) maps to -1000 - code, here only
    }
} // namespace mbavo
